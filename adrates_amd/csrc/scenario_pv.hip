// Scenario revaluation: the PV of every trade of a batch under S discount curves that share one knot grid
// (adr_scenario_pv*; declarations, semantics and the order of the book sum: include/adrates.h).
//
// pv[i][s] is what adr_price(VALUE) returns for trade i on the curve (times, dfs[s]): the fixed flows
// fix_sign * pay * D_s(tp) and the float coupons flt_sign * N * w * ((D_s(ts) / D_s(te) - 1) + spread * alpha) * D_s(tp),
// D_s(t) being InterpolatorAd.simple_interpolate (simple_interp.hpp).  No rates and no Jacobians are involved.
//
// Layout, lookup form, lane broadcast and book sum: scenario_common.hpp; the coupon description (Slot), make_slot,
// apply_slot, lane_slot and trade_pv: scenario_trade_slots.hpp, shared with xccy_scenario_pv.hip.  The group's table
// tab[k][lane] holds ln d under the log-linear schemes and d under LINEAR_FWD_RATES; a lane reads consecutive doubles, so a
// knot costs one conflict-free ds_read_b64.
//
// Everything about a date that does not depend on the scenario is computed once per wave.  The knot search is not
// done by a scalar loop per date (nine dependent LDS reads each) but lane-parallel: lane l describes coupon l of the
// trade - the segment searches of its dates (si::log_weights / si::locate), the two knot indices and weights - and marks
// the dates that need no evaluation of their own: an accrual start equal to the previous coupon's accrual end, a payment
// time equal to the accrual end (no payment lag), a fixed payment time equal to the float payment time of the same
// index.  The wave then walks the coupons in order, fetching coupon j's description from lane j with v_readlane (into
// scalar registers: every branch on it is uniform), and each lane evaluates D_s at the dates that are left: one exp of
// wa * L[a] + wb * L[b] per DISTINCT date under the log schemes, none under LINEAR_FWD_RATES.  An OIS with m annual
// coupons on both legs costs m + 1 exponentials per scenario instead of 3 m.
//
// The host twin (adr_scenario_pv_host) runs the same per-date and per-coupon code in the same order on CPU threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "host_pool.hpp"
#include "scenario_common.hpp"
#include "scenario_trade_slots.hpp"
#include "subbook.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace scen {

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    TradesDev tr;
    const double *times, *dfs;       // [K], [S][K]
    int K, S, method;
    int64_t n_chunks;                // kSub: the rows `work` holds, an upper bound of the plan's count
    double *pv, *work;               // [n][S] or null; [n_chunks][S]
    const int64_t *sub_chunks, *sub_bounds;      // kSub: the plan's chunk count and its [chunks][2] trade bounds (subbook.hpp)
};

// kSub: the chunks are those of a sub-book plan (their trade bounds come from a table) instead of ch * kChunk.
template <bool kLog, bool kLds, bool kSub>
__global__ __launch_bounds__(kThreads) void scenario_pv_kernel(Args a) {
    extern __shared__ double lds[];
    double* s_x = lds;                               // [K]
    double* s_tab = lds + a.K;                       // [K][64] (kLds)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = a.K, S = a.S;
    const int64_t s = static_cast<int64_t>(blockIdx.y) * kWave + lane;
    const bool live = s < S;
    const double* row = a.dfs + (live ? s : S - 1) * K;     // padding lanes price the last scenario and store nothing
    for (int k = threadIdx.x; k < K; k += kThreads) s_x[k] = a.times[k];
    if (kLds)
        for (int k = wave; k < K; k += kWaves) s_tab[k * kWave + lane] = kLog ? log(row[k]) : row[k];
    __syncthreads();
    const DevTab<kLog, kLds> tab{kLds ? s_tab + lane : row};
    const bool weighted = a.tr.flt_weight != nullptr;
    const Grid grid{s_x, K, a.method};
    int64_t n_chunks = a.n_chunks;
    if (kSub) {
        const int64_t planned = *a.sub_chunks;              // uniform: a scalar load
        n_chunks = planned < n_chunks ? planned : n_chunks;
    }
    for (int64_t ch = static_cast<int64_t>(blockIdx.x) * kWaves + wave; ch < n_chunks;
         ch += static_cast<int64_t>(gridDim.x) * kWaves) {
        const ChunkRange r = chunk_range<kSub>(ch, a.sub_bounds, a.tr.n);
        double book = 0.0;
        for (int64_t i = r.i0; i < r.i1; ++i) {
            const TradeHeader h = a.tr.header[i];           // uniform: scalar loads
            const Legs g{a.tr.fix_tp, a.tr.fix_pay, a.tr.flt_tp, a.tr.flt_ts, a.tr.flt_te, a.tr.flt_alpha, a.tr.flt_weight,
                         h.fix_begin, h.flt_begin, h.n_fix, h.n_flt, h.spread};
            const int m = h.n_fix > h.n_flt ? h.n_fix : h.n_flt;
            Acc acc{0.0, 0.0, 0.0};
            for (int base = 0; base < m; base += kWave) {
                const int cnt = m - base < kWave ? m - base : kWave;
                Slot mine;
                mine.flags = 0;
                mine.ws = mine.we = mine.wp = mine.wx = DateW{0, 0, 0.0, 0.0};
                mine.sa = 0.0; mine.w = 1.0; mine.pay = 0.0;
                if (lane < cnt) mine = make_slot<kLog, false>(g, base + lane, grid, grid);
                for (int j = 0; j < cnt; ++j) apply_slot<kLog>(lane_slot(mine, j, weighted), weighted, tab, tab, acc);
            }
            const double pv = trade_pv(acc, static_cast<double>(h.fix_sign), static_cast<double>(h.flt_sign), h.notional);
            if (a.pv && live) a.pv[i * S + s] = pv;
            book = book + pv;
        }
        if (live) a.work[ch * S + s] = book;
    }
}

// -------------------------------------------------------------------------------------------------------------- host
inline size_t lds_bytes(int K, bool table) { return (static_cast<size_t>(K) + (table ? static_cast<size_t>(K) * kWave : 0)) * sizeof(double); }

int validate(const std::string& w, int method, int K, int S, int64_t n, const void* times, const void* dfs, const void* book) {
    const int rc = check_scheme_knots(w, method, K);
    if (rc != ADR_OK) return rc;
    if (S < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one scenario is needed");
    if (n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one trade is needed");
    if (!times || !dfs) return adr_set_error(ADR_ERR_INVALID, w + ": null curve arrays");
    if (!book) return adr_set_error(ADR_ERR_INVALID, w + ": book_pv is NULL");
    return ADR_OK;
}

template <bool kLog, bool kLds>
hipError_t launch(const Args& a, dim3 grid, hipStream_t stream) {
    const size_t lds = lds_bytes(a.K, kLds);
    if (a.sub_bounds) return launch_with_lds(&scenario_pv_kernel<kLog, kLds, true>, a, lds, grid, stream);
    return launch_with_lds(&scenario_pv_kernel<kLog, kLds, false>, a, lds, grid, stream);
}

// The two kernels on `stream`; every pointer is device memory.  B > 0: the chunks of the sub-book plan `plan`, and
// `book` is sub_pv[B][S].
int enqueue(const std::string& w, adr_ctx* ctx, int method, int K, const double* times, int S, const double* dfs,
            const adr_trades* trades, double* pv, double* book, double* work, hipStream_t stream_or_null, int64_t B = 0,
            const int64_t* plan = nullptr) {
    const adr_ctx* owner = nullptr;
    const TradesDev* tr = adr_trades_device_view(trades, &owner);
    if (!tr) return adr_set_error(ADR_ERR_INVALID, w + ": null trades");
    if (owner != ctx) return adr_set_error(ADR_ERR_INVALID, w + ": the trades belong to another ctx");
    int rc = validate(w, method, K, S, tr->n, times, dfs, book);
    if (rc != ADR_OK) return rc;
    if (!work) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_scenario_pv_work doubles are needed)");
    const bool subs = B != 0 || plan;
    if (subs && B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    if (subs && !plan) return adr_set_error(ADR_ERR_INVALID, w + ": the sub-book plan is NULL (adr_scenario_subbook_plan fills it)");
    hipStream_t stream = nullptr;
    rc = call::target_stream(w, ctx, stream_or_null, &stream);
    if (rc != ADR_OK) return rc;
    const int64_t chunks = subs ? sub::max_chunks(tr->n, B, kChunk) : (tr->n + kChunk - 1) / kChunk;
    dim3 grid;
    rc = launch_grid(w, ctx, chunks, S, &grid);
    if (rc != ADR_OK) return rc;
    const sub::Plan pl = subs ? sub::plan_view(plan, B) : sub::Plan{nullptr, nullptr};
    const Args a{*tr, times, dfs, K, S, method, chunks, pv, work, subs ? pl.chunk_off + B : nullptr, pl.bounds};
    const bool in_lds = lds_bytes(K, true) <= kLdsBudget;
    const bool lin = method == ADR_INTERP_LINEAR_FWD_RATES;
    hipError_t e;
    if (lin) e = in_lds ? launch<false, true>(a, grid, stream) : launch<false, false>(a, grid, stream);
    else e = in_lds ? launch<true, true>(a, grid, stream) : launch<true, false>(a, grid, stream);
    if (e == hipSuccess && subs) e = sub::enqueue_sum(work, pl.chunk_off, chunks, B, S, book, stream);
    else if (e == hipSuccess) e = enqueue_book_sum(work, chunks, S, book, stream);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// What a sub-book call adds to the blocking form: the offsets (host), and, with k > 0, the tail measures of the rows
// in place of the rows themselves (book is then not written).
struct SubRequest {
    int64_t B;
    const int64_t* sub_off;
    int base_col, k;
    double *var, *es;
};

// Blocking form: outputs and scratch in one device allocation; the curves are copied in when they are host arrays.
// sub: `book` is sub_pv[B][S].
int run_blocking(const std::string& w, adr_ctx* ctx, int method, int K, const double* times, int S, const double* dfs,
                 bool curves_on_host, const adr_trades* trades, double* pv, double* book, const SubRequest* sub = nullptr) {
    const int64_t n = adr_trades_count(trades);
    const bool tail = sub && sub->k > 0;
    int rc = validate(w, method, K, S, trades ? n : 1, times, dfs, tail ? static_cast<const void*>(sub->var) : book);
    if (rc == ADR_OK && curves_on_host) rc = check_curves(w, K, times, S, dfs, "scenario");
    if (rc != ADR_OK) return rc;
    if (!trades) return adr_set_error(ADR_ERR_INVALID, w + ": null trades");
    std::vector<int64_t> plan;
    if (sub) {
        rc = sub::build_plan(w, n, sub->B, sub->sub_off, plan);
        if (rc == ADR_OK && tail) rc = sub::check_tail(w, sub->B, S, sub->base_col, sub->k);
        if (rc == ADR_OK && tail && !sub->es) rc = adr_set_error(ADR_ERR_INVALID, w + ": es is NULL");
        if (rc != ADR_OK) return rc;
    }
    const size_t B = sub ? static_cast<size_t>(sub->B) : 0, rows = sub ? B : 1;
    hipStream_t stream = nullptr;
    rc = call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *ht, *hd, *dpv, *dbook, *dwork, *dvar, *des;
    int64_t* dplan;
    call::Staging mem;                              // `plan` is uploaded from where it stands: it outlives finish()
    mem.in(&ht, times, K, curves_on_host);
    mem.in(&hd, dfs, static_cast<size_t>(S) * K, curves_on_host);
    mem.out(&dpv, pv, static_cast<size_t>(n) * S, pv != nullptr);
    if (tail) mem.scratch(&dbook, rows * S);        // the rows stay on the device: var and es go back in their place
    else mem.out(&dbook, book, rows * S);
    mem.scratch(&dwork, static_cast<size_t>(sub ? adr_scenario_subbook_work(n, sub->B, S) : adr_scenario_pv_work(n, S)));
    mem.in(&dplan, plan.data(), plan.size());
    mem.out(&dvar, tail ? sub->var : nullptr, B, tail);
    mem.out(&des, tail ? sub->es : nullptr, B, tail);
    hipError_t e = mem.begin(stream);
    if (e == hipSuccess)
        rc = enqueue(w, ctx, method, K, curves_on_host ? ht : times, S, curves_on_host ? hd : dfs, trades, dpv, dbook, dwork, stream,
                     sub ? sub->B : 0, dplan);
    if (e == hipSuccess && rc == ADR_OK && tail) e = sub::enqueue_tail(dbook, sub->B, S, sub->base_col, sub->k, dvar, des, stream);
    return mem.finish(w, rc, e, stream);
}

}  // namespace scen
}  // namespace adr

namespace SC = adr::scen;

extern "C" {

int64_t adr_scenario_pv_work(int64_t n, int S) {
    if (n < 1 || S < 1) return 0;
    return (n + SC::kChunk - 1) / SC::kChunk * S;
}

int adr_scenario_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S, const double* dfs_dev,
                        const adr_trades* trades, double* pv_dev, double* book_pv_dev, double* work_dev, void* stream) {
    return SC::enqueue("adr_scenario_pv_dev", ctx, interp_method, K, times_dev, S, dfs_dev, trades, pv_dev, book_pv_dev, work_dev,
                       static_cast<hipStream_t>(stream));
}

int adr_scenario_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S, const double* dfs,
                    const adr_trades* trades, double* pv, double* book_pv) {
    return SC::run_blocking("adr_scenario_pv", ctx, interp_method, K, times, S, dfs, true, trades, pv, book_pv);
}

int adr_curve_set_arrays(const adr_curve_set* set, int* interp_method, int* K, int* S, const double** times_dev,
                         const double** dfs_dev) {
    const adr_ctx* owner = nullptr;
    int m = 0, k = 0, s = 0;
    const double *t = nullptr, *d = nullptr;
    const int rc = adr_curve_set_device_view(set, &owner, &m, &k, &s, &t, &d);
    if (rc != ADR_OK) return rc;
    if (interp_method) *interp_method = m;
    if (K) *K = k;
    if (S) *S = s;
    if (times_dev) *times_dev = t;
    if (dfs_dev) *dfs_dev = d;
    return ADR_OK;
}

int adr_scenario_pv_set(adr_ctx* ctx, const adr_curve_set* set, const adr_trades* trades, double* pv, double* book_pv) {
    const std::string w = "adr_scenario_pv_set";
    SC::SetCurves c;
    const int rc = SC::curve_set_curves(w, ctx, set, &c);
    if (rc != ADR_OK) return rc;
    return SC::run_blocking(w, ctx, c.method, c.K, c.times, c.S, c.dfs, false, trades, pv, book_pv);
}

// The host entries' body; B > 0: book_pv is sub_pv[B][S] of the sub-books sub_off.
static int scenario_host_run(const std::string& w, int interp_method, int K, const double* times, int S, const double* dfs,
                             const SC::HostBatch& t, double* pv, double* book_pv, int n_threads, int64_t B, const int64_t* sub_off) {
    const int64_t n = t.n;
    int rc = SC::validate(w, interp_method, K, S, n, times, dfs, book_pv);
    if (rc == ADR_OK) rc = SC::check_curves(w, K, times, S, dfs, "scenario");
    if (rc != ADR_OK) return rc;
    rc = SC::check_host_batch(w, t);
    if (rc != ADR_OK) return rc;
    const SC::Grid grid{times, K, interp_method};
    return SC::host_book_run<false>(w, grid, S, dfs, grid, S, dfs, S, t, pv, book_pv, n_threads, B, sub_off);
}

int adr_scenario_pv_host(int interp_method, int K, const double* times, int S, const double* dfs, int64_t n,
                         const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                         const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                         const double* flt_weight, const double* notional, const double* spread, const double* fix_sign,
                         const double* flt_sign, double* pv, double* book_pv, int n_threads) {
    const SC::HostBatch t{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional, spread,
                          fix_sign, flt_sign};
    return scenario_host_run("adr_scenario_pv_host", interp_method, K, times, S, dfs, t, pv, book_pv, n_threads, 0, nullptr);
}

int adr_scenario_subbook_pv_host(int interp_method, int K, const double* times, int S, const double* dfs, int64_t n,
                                 const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                                 const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                                 const double* flt_weight, const double* notional, const double* spread, const double* fix_sign,
                                 const double* flt_sign, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv,
                                 int n_threads) {
    const std::string w = "adr_scenario_subbook_pv_host";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const SC::HostBatch t{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional, spread,
                          fix_sign, flt_sign};
    return scenario_host_run(w, interp_method, K, times, S, dfs, t, pv, sub_pv, n_threads, B, sub_off);
}

int adr_scenario_subbook_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S, const double* dfs,
                            const adr_trades* trades, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv) {
    const SC::SubRequest sub{B, sub_off, -1, 0, nullptr, nullptr};
    return SC::run_blocking("adr_scenario_subbook_pv", ctx, interp_method, K, times, S, dfs, true, trades, pv, sub_pv, &sub);
}

int adr_scenario_subbook_var_es(adr_ctx* ctx, int interp_method, int K, const double* times, int S, const double* dfs,
                                const adr_trades* trades, int64_t B, const int64_t* sub_off, int base_col, int k, double* var,
                                double* es) {
    const std::string w = "adr_scenario_subbook_var_es";
    if (k < 1) return adr_set_error(ADR_ERR_INVALID, w + ": k must be at least 1");
    const SC::SubRequest sub{B, sub_off, base_col, k, var, es};
    return SC::run_blocking(w, ctx, interp_method, K, times, S, dfs, true, trades, nullptr, nullptr, &sub);
}

int adr_scenario_subbook_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S, const double* dfs_dev,
                                const adr_trades* trades, int64_t B, const int64_t* plan_dev, double* pv_dev, double* sub_pv_dev,
                                double* work_dev, void* stream) {
    const std::string w = "adr_scenario_subbook_pv_dev";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    return SC::enqueue(w, ctx, interp_method, K, times_dev, S, dfs_dev, trades, pv_dev, sub_pv_dev, work_dev,
                       static_cast<hipStream_t>(stream), B, plan_dev);
}

int adr_scenario_subbook_pv_set(adr_ctx* ctx, const adr_curve_set* set, const adr_trades* trades, int64_t B, const int64_t* sub_off,
                                double* pv, double* sub_pv) {
    const std::string w = "adr_scenario_subbook_pv_set";
    SC::SetCurves c;
    const int rc = SC::curve_set_curves(w, ctx, set, &c);
    if (rc != ADR_OK) return rc;
    const SC::SubRequest sub{B, sub_off, -1, 0, nullptr, nullptr};
    return SC::run_blocking(w, ctx, c.method, c.K, c.times, c.S, c.dfs, false, trades, pv, sub_pv, &sub);
}

}  // extern "C"
