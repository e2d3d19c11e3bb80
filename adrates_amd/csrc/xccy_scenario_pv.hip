// Cross-currency scenario revaluation: the PV of the foreign leg of every cross-currency swap of a batch under S
// scenarios, each a pair of a foreign OIS row (the forwards) and an XCCY row (the discount factors)
// (adr_xccy_scenario_pv*; declarations, semantics and the order of the book sum: include/adrates.h).
//
// pv[i][s] = fix_sign * sum_j pay_j Dx_s(tp_j) [tp_j > 0]
//          + flt_sign * N * sum_j w_j ((Df_s(ts_j) / Df_s(te_j) - 1) [alpha_j > 0] + spread alpha_j) Dx_s(tp_j) [tp_j >= 0]:
// Df_s is InterpolatorAd.simple_interpolate on (times_f, dfs_f[s]), Dx_s the same rule on (times_x, dfs_x[s]).  The
// coupon description, its masks, the per-trade sum order and trade_pv are scenario_pv.hip's (scenario_trade_slots.hpp,
// kTwo = true: an accrual date is searched on the foreign grid, a payment date on the XCCY grid, and D(tp) is never taken
// from D(te)); layout, lookup form, lane broadcast and book sum: scenario_common.hpp.
//
// LDS rule.  The two knot grids always sit in LDS (at most 2 * 4096 doubles).  The tables ftab[k][lane], xtab[k][lane]:
//   1. both in LDS when grids + both tables fit kLdsBudget;
//   2. otherwise the SMALLER table (fewer knots; the foreign one on a tie: it is read twice per coupon) in LDS when grids +
//      that table fit, and every lane reads the other curve from its scenario's global row (taking ln per read under the
//      log schemes);
//   3. otherwise neither.
// The mode changes where a knot value is read, never the value or the arithmetic: results have the same bits in all three.
//
// Scheme pairs: both curves on LINEAR_FWD_RATES, or each on FLAT_FWD_RATES or LINEAR_ZERO_RATES (four pairs).
// LINEAR_FWD_RATES beside a log scheme is ADR_ERR_UNSUPPORTED, as in adr_price_xccy_foreign: the kernel is built with ONE
// table form (d or ln d) for both curves.
//
// A shared curve (S_f = 1 or S_x = 1: "not shocked") is read with row stride 0.  The host twin
// (adr_xccy_scenario_pv_host) runs the same per-date and per-coupon code in the same order on CPU threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "scenario_common.hpp"
#include "scenario_trade_slots.hpp"
#include "subbook.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace xscen {

using namespace scen;    // the shared pieces (scenario_common.hpp, scenario_trade_slots.hpp)

struct Curve {           // one side of a scenario pair
    int method, K;
    const double* times; // [K]
    int rows;            // 1 (shared) or S
    const double* dfs;   // [rows][K]
};

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    TradesDev tr;
    const double *f_times, *f_dfs, *x_times, *x_dfs;
    int Kf, Kx, S, fm, xm;
    int f_stride, x_stride;          // Kf / Kx, or 0 for a shared row
    int64_t n_chunks;                // kSub: the rows `work` holds, an upper bound of the plan's count
    double *pv, *work;               // [n][S] or null; [n_chunks][S]
    const int64_t *sub_chunks, *sub_bounds;      // kSub: the plan's chunk count and its [chunks][2] trade bounds (subbook.hpp)
};

// kSub: the chunks are those of a sub-book plan (their trade bounds come from a table) instead of ch * kChunk.
template <bool kLog, bool kFLds, bool kXLds, bool kSub>
__global__ __launch_bounds__(kThreads) void xccy_scenario_pv_kernel(Args a) {
    extern __shared__ double lds[];
    const int Kf = a.Kf, Kx = a.Kx, S = a.S;
    double* s_fx = lds;                                      // [Kf]
    double* s_xx = s_fx + Kf;                                // [Kx]
    double* s_ftab = s_xx + Kx;                              // [Kf][64] (kFLds)
    double* s_xtab = s_ftab + (kFLds ? Kf * kWave : 0);      // [Kx][64] (kXLds)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t s = static_cast<int64_t>(blockIdx.y) * kWave + lane;
    const bool live = s < S;
    const int64_t sr = live ? s : S - 1;                    // padding lanes price the last scenario and store nothing
    const double* frow = a.f_dfs + sr * a.f_stride;
    const double* xrow = a.x_dfs + sr * a.x_stride;
    for (int k = threadIdx.x; k < Kf; k += kThreads) s_fx[k] = a.f_times[k];
    for (int k = threadIdx.x; k < Kx; k += kThreads) s_xx[k] = a.x_times[k];
    if (kFLds)
        for (int k = wave; k < Kf; k += kWaves) s_ftab[k * kWave + lane] = kLog ? log(frow[k]) : frow[k];
    if (kXLds)
        for (int k = wave; k < Kx; k += kWaves) s_xtab[k * kWave + lane] = kLog ? log(xrow[k]) : xrow[k];
    __syncthreads();
    const DevTab<kLog, kFLds> ftab{kFLds ? s_ftab + lane : frow};
    const DevTab<kLog, kXLds> xtab{kXLds ? s_xtab + lane : xrow};
    const Grid fwd{s_fx, Kf, a.fm}, dsc{s_xx, Kx, a.xm};
    const bool weighted = a.tr.flt_weight != nullptr;
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
                if (lane < cnt) mine = make_slot<kLog, true>(g, base + lane, fwd, dsc);
                for (int j = 0; j < cnt; ++j) apply_slot<kLog>(lane_slot(mine, j, weighted), weighted, ftab, xtab, acc);
            }
            const double pv = trade_pv(acc, static_cast<double>(h.fix_sign), static_cast<double>(h.flt_sign), h.notional);
            if (a.pv && live) a.pv[i * S + s] = pv;
            book = book + pv;
        }
        if (live) a.work[ch * S + s] = book;
    }
}

// -------------------------------------------------------------------------------------------------------------- host
inline size_t lds_bytes(int Kf, int Kx, bool f_table, bool x_table) {
    return (static_cast<size_t>(Kf) + Kx + (f_table ? static_cast<size_t>(Kf) * kWave : 0) +
            (x_table ? static_cast<size_t>(Kx) * kWave : 0)) * sizeof(double);
}

// The LDS rule of the source header.
inline void lds_mode(int Kf, int Kx, bool* f_table, bool* x_table) {
    *f_table = *x_table = false;
    if (lds_bytes(Kf, Kx, true, true) <= kLdsBudget) *f_table = *x_table = true;
    else if (Kf <= Kx && lds_bytes(Kf, Kx, true, false) <= kLdsBudget) *f_table = true;
    else if (Kx < Kf && lds_bytes(Kf, Kx, false, true) <= kLdsBudget) *x_table = true;
}

int validate(const std::string& w, const Curve& f, const Curve& x, int S, int64_t n, const void* book) {
    int rc = check_scheme_knots(w, f.method, f.K);
    if (rc == ADR_OK) rc = check_scheme_knots(w, x.method, x.K);
    if (rc != ADR_OK) return rc;
    if ((f.method == ADR_INTERP_LINEAR_FWD_RATES) != (x.method == ADR_INTERP_LINEAR_FWD_RATES))
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": LINEAR_FWD_RATES (2) on one curve and a log-linear scheme on the other");
    if (S < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one scenario is needed");
    if ((f.rows != 1 && f.rows != S) || (x.rows != 1 && x.rows != S))
        return adr_set_error(ADR_ERR_INVALID, w + ": S_f and S_x must each be 1 (a shared curve) or S");
    if (n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one trade is needed");
    if (!f.times || !f.dfs || !x.times || !x.dfs) return adr_set_error(ADR_ERR_INVALID, w + ": null curve arrays");
    if (!book) return adr_set_error(ADR_ERR_INVALID, w + ": book_pv is NULL");
    return ADR_OK;
}

int check_host_curves(const std::string& w, const Curve& f, const Curve& x) {
    const int rc = check_curves(w, f.K, f.times, f.rows, f.dfs, "foreign row");
    return rc != ADR_OK ? rc : check_curves(w, x.K, x.times, x.rows, x.dfs, "XCCY row");
}

template <bool kLog, bool kFLds, bool kXLds>
hipError_t launch(const Args& a, dim3 grid, hipStream_t stream) {
    const size_t lds = lds_bytes(a.Kf, a.Kx, kFLds, kXLds);
    if (a.sub_bounds) return launch_with_lds(&xccy_scenario_pv_kernel<kLog, kFLds, kXLds, true>, a, lds, grid, stream);
    return launch_with_lds(&xccy_scenario_pv_kernel<kLog, kFLds, kXLds, false>, a, lds, grid, stream);
}

template <bool kLog>
hipError_t launch_mode(const Args& a, bool f_table, bool x_table, dim3 grid, hipStream_t stream) {
    if (f_table && x_table) return launch<kLog, true, true>(a, grid, stream);
    if (f_table) return launch<kLog, true, false>(a, grid, stream);
    if (x_table) return launch<kLog, false, true>(a, grid, stream);
    return launch<kLog, false, false>(a, grid, stream);
}

// The two kernels on `stream`; every pointer is device memory.  B > 0: the chunks of the sub-book plan `plan`, and
// `book` is sub_pv[B][S].
int enqueue(const std::string& w, adr_ctx* ctx, const Curve& f, const Curve& x, int S, const adr_trades* legs, double* pv,
            double* book, double* work, hipStream_t stream_or_null, int64_t B = 0, const int64_t* plan = nullptr) {
    const adr_ctx* owner = nullptr;
    const TradesDev* tr = adr_trades_device_view(legs, &owner);
    if (!tr) return adr_set_error(ADR_ERR_INVALID, w + ": null trades");
    if (owner != ctx) return adr_set_error(ADR_ERR_INVALID, w + ": the trades belong to another ctx");
    int rc = validate(w, f, x, S, tr->n, book);
    if (rc != ADR_OK) return rc;
    if (!work) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_xccy_scenario_pv_work doubles are needed)");
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
    const Args a{*tr, f.times, f.dfs, x.times, x.dfs, f.K, x.K, S, f.method, x.method, f.rows == 1 ? 0 : f.K,
                 x.rows == 1 ? 0 : x.K, chunks, pv, work, subs ? pl.chunk_off + B : nullptr, pl.bounds};
    bool f_table, x_table;
    lds_mode(f.K, x.K, &f_table, &x_table);
    hipError_t e = f.method == ADR_INTERP_LINEAR_FWD_RATES ? launch_mode<false>(a, f_table, x_table, grid, stream)
                                                           : launch_mode<true>(a, f_table, x_table, grid, stream);
    if (e == hipSuccess && subs) e = sub::enqueue_sum(work, pl.chunk_off, chunks, B, S, book, stream);
    else if (e == hipSuccess) e = enqueue_book_sum(work, chunks, S, book, stream);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// Blocking form: the curves, the outputs and the scratch in one device allocation.  B > 0: `book` is sub_pv[B][S] of the
// sub-books sub_off (host), and the plan is built and uploaded here.
int run_blocking(const std::string& w, adr_ctx* ctx, const Curve& f, const Curve& x, int S, const adr_trades* legs, double* pv,
                 double* book, int64_t B = 0, const int64_t* sub_off = nullptr) {
    const int64_t n = adr_trades_count(legs);
    int rc = validate(w, f, x, S, legs ? n : 1, book);
    if (rc == ADR_OK) rc = check_host_curves(w, f, x);
    if (rc != ADR_OK) return rc;
    if (!legs) return adr_set_error(ADR_ERR_INVALID, w + ": null trades");
    std::vector<int64_t> plan;
    if (B > 0) {
        rc = sub::build_plan(w, n, B, sub_off, plan);
        if (rc != ADR_OK) return rc;
    }
    hipStream_t stream = nullptr;
    rc = call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const size_t rows = B > 0 ? static_cast<size_t>(B) : 1;
    double *dft, *dfd, *dxt, *dxd, *dpv, *dbook, *dwork;
    int64_t* dplan;
    call::Staging mem;                              // `plan` is uploaded from where it stands: it outlives finish()
    mem.in(&dft, f.times, f.K);
    mem.in(&dfd, f.dfs, static_cast<size_t>(f.rows) * f.K);
    mem.in(&dxt, x.times, x.K);
    mem.in(&dxd, x.dfs, static_cast<size_t>(x.rows) * x.K);
    mem.in(&dplan, plan.data(), plan.size());
    mem.out(&dpv, pv, static_cast<size_t>(n) * S, pv != nullptr);
    mem.out(&dbook, book, rows * S);
    mem.scratch(&dwork, static_cast<size_t>(B > 0 ? adr_scenario_subbook_work(n, B, S) : adr_xccy_scenario_pv_work(n, S)));
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess)
        rc = enqueue(w, ctx, Curve{f.method, f.K, dft, f.rows, dfd}, Curve{x.method, x.K, dxt, x.rows, dxd}, S, legs, dpv, dbook,
                     dwork, stream, B, dplan);
    return mem.finish(w, rc, e, stream);
}

// The host entries' body; B > 0: book is sub_pv[B][S] of the sub-books sub_off.
int host_run(const std::string& w, const Curve& f, const Curve& x, int S, const HostBatch& t, double* pv, double* book,
             int n_threads, int64_t B = 0, const int64_t* sub_off = nullptr) {
    int rc = validate(w, f, x, S, t.n, book);
    if (rc == ADR_OK) rc = check_host_curves(w, f, x);
    if (rc == ADR_OK) rc = check_host_batch(w, t);
    if (rc != ADR_OK) return rc;
    return host_book_run<true>(w, Grid{f.times, f.K, f.method}, f.rows, f.dfs, Grid{x.times, x.K, x.method}, x.rows, x.dfs, S, t,
                               pv, book, n_threads, B, sub_off);
}

}  // namespace xscen
}  // namespace adr

namespace XS = adr::xscen;

extern "C" {

int64_t adr_xccy_scenario_pv_work(int64_t n, int S) { return adr_scenario_pv_work(n, S); }     // the same chunks

int adr_xccy_scenario_pv_dev(adr_ctx* ctx, int for_method, int K_f, const double* times_f_dev, int S_f, const double* dfs_f_dev,
                             int x_method, int K_x, const double* times_x_dev, int S_x, const double* dfs_x_dev, int S,
                             const adr_trades* legs, double* pv_dev, double* book_pv_dev, double* work_dev, void* stream) {
    return XS::enqueue("adr_xccy_scenario_pv_dev", ctx, XS::Curve{for_method, K_f, times_f_dev, S_f, dfs_f_dev},
                       XS::Curve{x_method, K_x, times_x_dev, S_x, dfs_x_dev}, S, legs, pv_dev, book_pv_dev, work_dev,
                       static_cast<hipStream_t>(stream));
}

int adr_xccy_scenario_pv(adr_ctx* ctx, int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f, int x_method,
                         int K_x, const double* times_x, int S_x, const double* dfs_x, int S, const adr_trades* legs, double* pv,
                         double* book_pv) {
    return XS::run_blocking("adr_xccy_scenario_pv", ctx, XS::Curve{for_method, K_f, times_f, S_f, dfs_f},
                            XS::Curve{x_method, K_x, times_x, S_x, dfs_x}, S, legs, pv, book_pv);
}

int adr_xccy_scenario_pv_host(int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f, int x_method, int K_x,
                              const double* times_x, int S_x, const double* dfs_x, int S, int64_t n, const int64_t* fix_off,
                              const int64_t* flt_off, const double* fix_tp, const double* fix_pay, const double* flt_tp,
                              const double* flt_ts, const double* flt_te, const double* flt_alpha, const double* flt_weight,
                              const double* notional, const double* spread, const double* fix_sign, const double* flt_sign,
                              double* pv, double* book_pv, int n_threads) {
    const adr::scen::HostBatch t{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional,
                                 spread, fix_sign, flt_sign};
    return XS::host_run("adr_xccy_scenario_pv_host", XS::Curve{for_method, K_f, times_f, S_f, dfs_f},
                        XS::Curve{x_method, K_x, times_x, S_x, dfs_x}, S, t, pv, book_pv, n_threads);
}

int adr_xccy_scenario_subbook_pv(adr_ctx* ctx, int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f,
                                 int x_method, int K_x, const double* times_x, int S_x, const double* dfs_x, int S,
                                 const adr_trades* legs, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv) {
    const std::string w = "adr_xccy_scenario_subbook_pv";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    return XS::run_blocking(w, ctx, XS::Curve{for_method, K_f, times_f, S_f, dfs_f}, XS::Curve{x_method, K_x, times_x, S_x, dfs_x}, S,
                            legs, pv, sub_pv, B, sub_off);
}

int adr_xccy_scenario_subbook_pv_dev(adr_ctx* ctx, int for_method, int K_f, const double* times_f_dev, int S_f,
                                     const double* dfs_f_dev, int x_method, int K_x, const double* times_x_dev, int S_x,
                                     const double* dfs_x_dev, int S, const adr_trades* legs, int64_t B, const int64_t* plan_dev,
                                     double* pv_dev, double* sub_pv_dev, double* work_dev, void* stream) {
    const std::string w = "adr_xccy_scenario_subbook_pv_dev";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    return XS::enqueue(w, ctx, XS::Curve{for_method, K_f, times_f_dev, S_f, dfs_f_dev},
                       XS::Curve{x_method, K_x, times_x_dev, S_x, dfs_x_dev}, S, legs, pv_dev, sub_pv_dev, work_dev,
                       static_cast<hipStream_t>(stream), B, plan_dev);
}

int adr_xccy_scenario_subbook_pv_host(int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f, int x_method,
                                      int K_x, const double* times_x, int S_x, const double* dfs_x, int S, int64_t n,
                                      const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                                      const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                                      const double* flt_weight, const double* notional, const double* spread,
                                      const double* fix_sign, const double* flt_sign, int64_t B, const int64_t* sub_off,
                                      double* pv, double* sub_pv, int n_threads) {
    const std::string w = "adr_xccy_scenario_subbook_pv_host";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const adr::scen::HostBatch t{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional,
                                 spread, fix_sign, flt_sign};
    return XS::host_run(w, XS::Curve{for_method, K_f, times_f, S_f, dfs_f}, XS::Curve{x_method, K_x, times_x, S_x, dfs_x}, S, t, pv,
                        sub_pv, n_threads, B, sub_off);
}

}  // extern "C"
