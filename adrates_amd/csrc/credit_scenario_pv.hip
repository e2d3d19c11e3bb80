// Credit scenario revaluation: the PV of every trade of a batch under S scenarios, each a PAIR of a discount curve row
// and a row of spread shocks per credit bucket (adr_credit_scenario_pv*; declarations, semantics and the order of the
// book sum: include/adrates.h).
//
// pv[i][s] is adr_scenario_pv's sum with every PAYMENT discount factor D_s(tp) replaced by D_s(tp) exp(-x tau),
// x = z[i] + dz[s][bucket[i]] (no shock when bucket[i] = -1), tau the flow's spread time.  The forward D_s(ts) / D_s(te)
// carries no spread.  Under the log-linear schemes ln D(tp) is a weighted sum of two table entries, so -x tau is added
// to the exponent and a bond flow still costs ONE exp; under LINEAR_FWD_RATES the factor is an exp of its own.
//
// Layout, lookup form, lane broadcast and book sum: scenario_common.hpp.  Beside the group's discount table the block
// holds the group's spread table dzt[g][lane], so x costs one conflict-free ds_read_b64 per trade.  Where the two do not
// fit together the small spread table stays in LDS and the lanes read their discount rows from global memory.  Lane l
// describes coupon l of the trade as in scenario_pv.hip (segment searches, knot indices and weights, the dates that need
// no evaluation of their own).
//
// A trade with z = 0 and bucket = -1 has no spread: that is uniform over the wave, and such a trade takes
// scenario_pv.hip's own coupon code behind a uniform branch (no tau is read, no factor formed).
//
// A shared row (S_disc = 1 or S_spr = 1: "not shocked") is read with row stride 0.  The host twin
// (adr_credit_scenario_pv_host) runs the same per-date and per-coupon code in the same order on CPU threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "host_pool.hpp"
#include "scenario_common.hpp"
#include "subbook.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace cscen {

using namespace scen;    // the shared pieces (scenario_common.hpp)

// ln D (kLog) or D on the table: the part of a discount factor before its exponential.
template <bool kLog, class Tab>
__host__ __device__ inline double raw_df(const DateW& d, const Tab& tab) {
    const double la = tab(d.a);
    if (kLog) {
        double s = d.wa * la;
        if (d.b != d.a) s = s + d.wb * tab(d.b);
        return s;
    }
    double f = la;
    if (d.b != d.a) f = la + d.wb * (tab(d.b) - la);
    return f;
}

template <bool kLog>
__host__ __device__ inline double plain_df(double raw) { return kLog ? exp(raw) : raw; }

// D exp(-xt): one exp under the log-linear schemes.
template <bool kLog>
__host__ __device__ inline double spread_df(double raw, double xt) { return kLog ? exp(raw - xt) : raw * exp(-xt); }

// Coupon index c of a trade: its float coupon (c < n_flt) and its fixed flow (c < n_fix).  The masks are adr_price's:
// a float coupon counts when tp >= 0 and has no forward when alpha <= 0, a fixed flow counts when tp > 0.
enum : int {
    kHasFlt = 1, kHasFix = 2,
    kTsIsPrevTe = 4,     // accrual start == the previous coupon's accrual end: D(ts) is the D(te) just computed
    kTpIsTe = 8,         // no payment lag: ln D(tp) is ln D(te)
    kFixIsFltTp = 16,    // the fixed flow is paid with the float coupon at the same spread time: its factor is the coupon's
    kNoAccrual = 32      // alpha <= 0: the coupon is spread * alpha * D(tp)
};

struct Slot {
    int flags;
    DateW ws, we, wp, wx;
    double sa, w, pay;   // spread * alpha, the coupon's notional multiplier, the fixed amount
    double tf, tx;       // the spread times of the float coupon and of the fixed flow (trades with a spread only)
};

__host__ __device__ inline Slot empty_slot() {
    Slot s;
    s.flags = 0;
    s.ws = s.we = s.wp = s.wx = DateW{0, 0, 0.0, 0.0};
    s.sa = 0.0; s.w = 1.0; s.pay = 0.0;
    s.tf = 0.0; s.tx = 0.0;
    return s;
}

struct Legs {            // one trade's cash flows
    const double *fix_tp, *fix_pay, *flt_tp, *flt_ts, *flt_te, *flt_alpha, *flt_weight, *fix_tau, *flt_tau;
    int64_t f0, l0;
    int n_fix, n_flt;
    double spread;
};

template <bool kLog>
__host__ __device__ inline Slot make_slot(const Legs& g, int c, bool spread_on, const double* x, int K, int method) {
    Slot s = empty_slot();
    double tp = 0.0;
    bool flt = false;
    if (c < g.n_flt) {
        const int64_t i = g.l0 + c;
        tp = g.flt_tp[i];
        flt = tp >= 0.0;
    }
    if (flt) {
        const int64_t i = g.l0 + c;
        const double ts = g.flt_ts[i], te = g.flt_te[i], al = g.flt_alpha[i];
        s.flags |= kHasFlt;
        s.sa = g.spread * al;
        if (g.flt_weight) s.w = g.flt_weight[i];
        if (spread_on) s.tf = g.flt_tau[i];
        if (al > 0.0) {
            // the previous coupon left its D(te) behind when it counted and accrued
            if (c > 0 && ts == g.flt_te[i - 1] && g.flt_tp[i - 1] >= 0.0 && g.flt_alpha[i - 1] > 0.0) s.flags |= kTsIsPrevTe;
            else s.ws = date_weights<kLog>(ts, x, K, method);
            s.we = date_weights<kLog>(te, x, K, method);
            if (tp == te) s.flags |= kTpIsTe;
            else s.wp = date_weights<kLog>(tp, x, K, method);
        } else {
            s.flags |= kNoAccrual;
            s.wp = date_weights<kLog>(tp, x, K, method);
        }
    }
    if (c < g.n_fix) {
        const int64_t i = g.f0 + c;
        const double xt = g.fix_tp[i];
        if (xt > 0.0) {
            s.flags |= kHasFix;
            s.pay = g.fix_pay[i];
            if (spread_on) s.tx = g.fix_tau[i];
            if (flt && xt == tp && s.tx == s.tf) s.flags |= kFixIsFltTp;
            else s.wx = date_weights<kLog>(xt, x, K, method);
        }
    }
    return s;
}

struct Acc {             // one scenario's running state inside a trade
    double de, flt, fix; // D(te) of the previous coupon; the legs' sums before sign and notional
};

// kSpread = false is scenario_pv.hip's coupon, expression for expression; x is the scenario's spread of this trade.
template <bool kLog, bool kSpread, class Tab>
__host__ __device__ inline void apply_slot(const Slot& s, bool weighted, const Tab& tab, double x, Acc& a) {
    double dp = 0.0;
    if (s.flags & kHasFlt) {
        double term;
        const double xt = kSpread ? x * s.tf : 0.0;
        if (s.flags & kNoAccrual) {
            const double rp = raw_df<kLog>(s.wp, tab);
            dp = kSpread ? spread_df<kLog>(rp, xt) : plain_df<kLog>(rp);
            term = s.sa * dp;
        } else {
            const double ds = (s.flags & kTsIsPrevTe) ? a.de : plain_df<kLog>(raw_df<kLog>(s.ws, tab));
            const double re = raw_df<kLog>(s.we, tab);
            const double de = plain_df<kLog>(re);
            if (kSpread) dp = spread_df<kLog>((s.flags & kTpIsTe) ? re : raw_df<kLog>(s.wp, tab), xt);
            else dp = (s.flags & kTpIsTe) ? de : plain_df<kLog>(raw_df<kLog>(s.wp, tab));
            term = ((ds / de - 1.0) + s.sa) * dp;
            a.de = de;
        }
        if (weighted) term = s.w * term;
        a.flt = a.flt + term;
    }
    if (s.flags & kHasFix) {
        double dx = dp;
        if (!(s.flags & kFixIsFltTp)) {
            const double rx = raw_df<kLog>(s.wx, tab);
            dx = kSpread ? spread_df<kLog>(rx, x * s.tx) : plain_df<kLog>(rx);
        }
        a.fix = a.fix + s.pay * dx;
    }
}

// + 0.0: as scenario_pv.hip's - the PV of a trade without a live flow is +0.0 whatever its signs.
__host__ __device__ inline double trade_pv(const Acc& a, double fix_sign, double flt_sign, double notional) {
    return (fix_sign * a.fix + (flt_sign * notional) * a.flt) + 0.0;
}

// A leg's range against the length of its spread-time array; false: nothing of the trade is read.
__host__ __device__ inline bool leg_fits(int64_t begin, int64_t count, int64_t total) {
    return begin >= 0 && count >= 0 && begin + count <= total;
}

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    TradesDev tr;
    const double *times, *dfs, *dz;  // [K], [S_disc][K], [S_spr][G]
    const double* z;                 // [n]
    const int32_t* bucket;           // [n]
    const double *fix_tau, *flt_tau; // [n_fix], [n_flt]
    int64_t n_fix, n_flt;
    int K, S, G, method;
    int disc_stride, dz_stride;      // K / G, or 0 for a shared row
    int64_t n_chunks;                // kSub: the rows `work` holds, an upper bound of the plan's count
    double *pv, *work;               // [n][S] or null; [n_chunks][S]
    const int64_t *sub_chunks, *sub_bounds;      // kSub: the plan's chunk count and its [chunks][2] trade bounds (subbook.hpp)
};

// Lane j's slot in scalar registers; only the parts its flags say will be read.
template <bool kSpread>
__device__ inline Slot lane_slot(const Slot& m, int j, bool weighted) {
    Slot u = empty_slot();
    u.flags = lane_int(m.flags, j);
    if (u.flags & kHasFlt) {
        if (!(u.flags & kNoAccrual)) {
            if (!(u.flags & kTsIsPrevTe)) u.ws = lane_date(m.ws, j);
            u.we = lane_date(m.we, j);
        }
        if (!(u.flags & kTpIsTe)) u.wp = lane_date(m.wp, j);
        u.sa = lane_dbl(m.sa, j);
        if (weighted) u.w = lane_dbl(m.w, j);
        if (kSpread) u.tf = lane_dbl(m.tf, j);
    }
    if (u.flags & kHasFix) {
        if (!(u.flags & kFixIsFltTp)) {
            u.wx = lane_date(m.wx, j);
            if (kSpread) u.tx = lane_dbl(m.tx, j);
        }
        u.pay = lane_dbl(m.pay, j);
    }
    return u;
}

// kSub: the chunks are those of a sub-book plan (their trade bounds come from a table) instead of ch * kChunk.
template <bool kLog, bool kLds, bool kSub>
__global__ __launch_bounds__(kThreads) void credit_scenario_pv_kernel(Args a) {
    extern __shared__ double lds[];
    const int K = a.K, S = a.S, G = a.G;
    double* s_x = lds;                               // [K]
    double* s_dz = s_x + K;                          // [G][64]
    double* s_tab = s_dz + G * kWave;                // [K][64] (kLds)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t s = static_cast<int64_t>(blockIdx.y) * kWave + lane;
    const bool live = s < S;
    const int64_t sr = live ? s : S - 1;                    // padding lanes price the last scenario and store nothing
    const double* row = a.dfs + sr * a.disc_stride;
    for (int k = threadIdx.x; k < K; k += kThreads) s_x[k] = a.times[k];
    for (int g = wave; g < G; g += kWaves) s_dz[g * kWave + lane] = a.dz[sr * a.dz_stride + g];
    if (kLds)
        for (int k = wave; k < K; k += kWaves) s_tab[k * kWave + lane] = kLog ? log(row[k]) : row[k];
    __syncthreads();
    const DevTab<kLog, kLds> tab{kLds ? s_tab + lane : row};
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
            const double z = a.z[i];
            const int bucket = a.bucket[i];
            const Legs g{a.tr.fix_tp, a.tr.fix_pay, a.tr.flt_tp, a.tr.flt_ts, a.tr.flt_te, a.tr.flt_alpha, a.tr.flt_weight,
                         a.fix_tau, a.flt_tau, h.fix_begin, h.flt_begin, h.n_fix, h.n_flt, h.spread};
            const bool ok = bucket >= -1 && bucket < G && leg_fits(h.fix_begin, h.n_fix, a.n_fix) &&
                            leg_fits(h.flt_begin, h.n_flt, a.n_flt);
            const int m = ok ? (h.n_fix > h.n_flt ? h.n_fix : h.n_flt) : 0;
            const bool spread_on = !(z == 0.0 && bucket == -1);
            Acc acc{0.0, 0.0, 0.0};
            if (spread_on) {
                const double x = z + ((ok && bucket >= 0) ? s_dz[bucket * kWave + lane] : 0.0);
                for (int base = 0; base < m; base += kWave) {
                    const int cnt = m - base < kWave ? m - base : kWave;
                    Slot mine = empty_slot();
                    if (lane < cnt) mine = make_slot<kLog>(g, base + lane, true, s_x, K, a.method);
                    for (int j = 0; j < cnt; ++j) apply_slot<kLog, true>(lane_slot<true>(mine, j, weighted), weighted, tab, x, acc);
                }
            } else {
                for (int base = 0; base < m; base += kWave) {
                    const int cnt = m - base < kWave ? m - base : kWave;
                    Slot mine = empty_slot();
                    if (lane < cnt) mine = make_slot<kLog>(g, base + lane, false, s_x, K, a.method);
                    for (int j = 0; j < cnt; ++j) apply_slot<kLog, false>(lane_slot<false>(mine, j, weighted), weighted, tab, 0.0, acc);
                }
            }
            // a bucket or a leg range that cannot be right: no reads, a NaN PV
            const double pv = ok ? trade_pv(acc, static_cast<double>(h.fix_sign), static_cast<double>(h.flt_sign), h.notional) : NAN;
            if (a.pv && live) a.pv[i * S + s] = pv;
            book = book + pv;
        }
        if (live) a.work[ch * S + s] = book;
    }
}

// -------------------------------------------------------------------------------------------------------------- host
// Knot times, the spread table and (table) the discount table: 8 (65 K + 64 G) bytes, so with G = 32 the discount table
// stays in LDS up to K = (20480 - 2048) / 65 = 283 knots, with G = 0 up to scenario_pv.hip's 315.
inline size_t lds_bytes(int K, int G, bool table) {
    return (static_cast<size_t>(K) + static_cast<size_t>(G) * kWave + (table ? static_cast<size_t>(K) * kWave : 0)) * sizeof(double);
}

struct Curves {          // the scalars and curve pointers of one call, host or device
    int method, K;
    const double* times;
    int S_disc;
    const double* dfs;
    int G, S_spr;
    const double* dz;
    int S;
};

struct Extra {           // what the trades carry besides the batch
    const double* z;
    const int32_t* bucket;
    int64_t n_fix;
    const double* fix_tau;
    int64_t n_flt;
    const double* flt_tau;
};

int validate(const std::string& w, const Curves& c, int64_t n, const Extra& x, const void* book) {
    const int rc = check_scheme_knots(w, c.method, c.K);
    if (rc != ADR_OK) return rc;
    if (c.G < 0 || c.G > ADR_CREDIT_MAX_BUCKETS)
        return adr_set_error(ADR_ERR_INVALID, w + ": 0 .. ADR_CREDIT_MAX_BUCKETS (32) spread buckets are allowed");
    if (c.S < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one scenario is needed");
    if ((c.S_disc != 1 && c.S_disc != c.S) || (c.S_spr != 1 && c.S_spr != c.S))
        return adr_set_error(ADR_ERR_INVALID, w + ": S_disc and S_spr must each be 1 (a shared row) or S");
    if (n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one trade is needed");
    if (!c.times || !c.dfs) return adr_set_error(ADR_ERR_INVALID, w + ": null curve arrays");
    if (c.G > 0 && !c.dz) return adr_set_error(ADR_ERR_INVALID, w + ": dz is NULL with G > 0");
    if (!x.z || !x.bucket) return adr_set_error(ADR_ERR_INVALID, w + ": z or bucket is NULL");
    if (x.n_fix < 0 || x.n_flt < 0 || x.n_fix > INT32_MAX || x.n_flt > INT32_MAX)
        return adr_set_error(ADR_ERR_INVALID, w + ": flow counts must lie in 0 .. 2^31 - 1");
    if ((x.n_fix > 0 && !x.fix_tau) || (x.n_flt > 0 && !x.flt_tau))
        return adr_set_error(ADR_ERR_INVALID, w + ": null spread-time array");
    if (!book) return adr_set_error(ADR_ERR_INVALID, w + ": book_pv is NULL");
    return ADR_OK;
}

// The host arrays of the spread side: finite z, dz and spread times, buckets inside -1 .. G - 1.
int check_spreads(const std::string& w, const Curves& c, int64_t n, const Extra& x) {
    for (int64_t i = 0; i < static_cast<int64_t>(c.S_spr) * c.G; ++i)
        if (!std::isfinite(c.dz[i]))
            return adr_set_error(ADR_ERR_INVALID, w + ": spread shocks must be finite (row " + std::to_string(i / c.G) +
                                                      ", bucket " + std::to_string(i % c.G) + ")");
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(x.z[i])) return adr_set_error(ADR_ERR_INVALID, w + ": spreads z must be finite (trade " + std::to_string(i) + ")");
        if (x.bucket[i] < -1 || x.bucket[i] >= c.G)
            return adr_set_error(ADR_ERR_INVALID, w + ": bucket " + std::to_string(x.bucket[i]) + " of trade " + std::to_string(i) +
                                                      " is outside -1 .. G - 1");
    }
    for (int64_t i = 0; i < x.n_fix; ++i)
        if (!std::isfinite(x.fix_tau[i])) return adr_set_error(ADR_ERR_INVALID, w + ": spread times must be finite (fixed flow " + std::to_string(i) + ")");
    for (int64_t i = 0; i < x.n_flt; ++i)
        if (!std::isfinite(x.flt_tau[i])) return adr_set_error(ADR_ERR_INVALID, w + ": spread times must be finite (float coupon " + std::to_string(i) + ")");
    return ADR_OK;
}

template <bool kLog, bool kLds>
hipError_t launch(const Args& a, dim3 grid, hipStream_t stream) {
    const size_t lds = lds_bytes(a.K, a.G, kLds);
    if (a.sub_bounds) return launch_with_lds(&credit_scenario_pv_kernel<kLog, kLds, true>, a, lds, grid, stream);
    return launch_with_lds(&credit_scenario_pv_kernel<kLog, kLds, false>, a, lds, grid, stream);
}

// The two kernels on `stream`; every pointer is device memory.  B > 0: the chunks of the sub-book plan `plan`, and
// `book` is sub_pv[B][S].
int enqueue(const std::string& w, adr_ctx* ctx, const Curves& c, const adr_trades* trades, const Extra& x, double* pv,
            double* book, double* work, hipStream_t stream_or_null, int64_t B = 0, const int64_t* plan = nullptr) {
    const adr_ctx* owner = nullptr;
    const TradesDev* tr = adr_trades_device_view(trades, &owner);
    if (!tr) return adr_set_error(ADR_ERR_INVALID, w + ": null trades");
    if (owner != ctx) return adr_set_error(ADR_ERR_INVALID, w + ": the trades belong to another ctx");
    int rc = validate(w, c, tr->n, x, book);
    if (rc != ADR_OK) return rc;
    if (!work) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_credit_scenario_pv_work doubles are needed)");
    const bool subs = B != 0 || plan;
    if (subs && B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    if (subs && !plan) return adr_set_error(ADR_ERR_INVALID, w + ": the sub-book plan is NULL (adr_scenario_subbook_plan fills it)");
    hipStream_t stream = nullptr;
    rc = call::target_stream(w, ctx, stream_or_null, &stream);
    if (rc != ADR_OK) return rc;
    const int64_t chunks = subs ? sub::max_chunks(tr->n, B, kChunk) : (tr->n + kChunk - 1) / kChunk;
    dim3 grid;
    rc = launch_grid(w, ctx, chunks, c.S, &grid);
    if (rc != ADR_OK) return rc;
    const sub::Plan pl = subs ? sub::plan_view(plan, B) : sub::Plan{nullptr, nullptr};
    const Args a{*tr, c.times, c.dfs, c.dz, x.z, x.bucket, x.fix_tau, x.flt_tau, x.n_fix, x.n_flt, c.K, c.S, c.G, c.method,
                 c.S_disc == 1 ? 0 : c.K, c.S_spr == 1 ? 0 : c.G, chunks, pv, work, subs ? pl.chunk_off + B : nullptr, pl.bounds};
    const bool in_lds = lds_bytes(c.K, c.G, true) <= kLdsBudget;
    const bool lin = c.method == ADR_INTERP_LINEAR_FWD_RATES;
    hipError_t e;
    if (lin) e = in_lds ? launch<false, true>(a, grid, stream) : launch<false, false>(a, grid, stream);
    else e = in_lds ? launch<true, true>(a, grid, stream) : launch<true, false>(a, grid, stream);
    if (e == hipSuccess && subs) e = sub::enqueue_sum(work, pl.chunk_off, chunks, B, c.S, book, stream);
    else if (e == hipSuccess) e = enqueue_book_sum(work, chunks, c.S, book, stream);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// Blocking form: inputs, outputs and scratch in one device allocation; the curves are copied in when they are host arrays.
// B > 0: `book` is sub_pv[B][S] of the sub-books sub_off (host).
int run_blocking(const std::string& w, adr_ctx* ctx, const Curves& c, bool curves_on_host, const adr_trades* trades,
                 const Extra& x, double* pv, double* book, int64_t B = 0, const int64_t* sub_off = nullptr) {
    const int64_t n = adr_trades_count(trades);
    int rc = validate(w, c, trades ? n : 1, x, book);
    if (rc == ADR_OK && curves_on_host) rc = check_curves(w, c.K, c.times, c.S_disc, c.dfs, "row");
    if (rc != ADR_OK) return rc;
    if (!trades) return adr_set_error(ADR_ERR_INVALID, w + ": null trades");
    rc = check_spreads(w, c, n, x);
    if (rc != ADR_OK) return rc;
    std::vector<int64_t> plan;
    if (B > 0) {
        rc = sub::build_plan(w, n, B, sub_off, plan);
        if (rc != ADR_OK) return rc;
    }
    const size_t rows = B > 0 ? static_cast<size_t>(B) : 1;
    hipStream_t stream = nullptr;
    rc = call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *ht, *hd, *ddz, *dzs, *dft, *dlt, *dpv, *dbook, *dwork;
    int64_t* dplan;
    int32_t* dbucket;
    call::Staging mem;                              // `plan` is uploaded from where it stands: it outlives finish()
    mem.in(&ht, c.times, c.K, curves_on_host);
    mem.in(&hd, c.dfs, static_cast<size_t>(c.S_disc) * c.K, curves_on_host);
    mem.in(&dplan, plan.data(), plan.size());
    mem.in(&ddz, c.dz, static_cast<size_t>(c.S_spr) * c.G);        // null with G = 0
    mem.in(&dzs, x.z, n);
    mem.in(&dft, x.fix_tau, x.n_fix);
    mem.in(&dlt, x.flt_tau, x.n_flt);
    mem.in(&dbucket, x.bucket, n);
    mem.out(&dpv, pv, static_cast<size_t>(n) * c.S, pv != nullptr);
    mem.out(&dbook, book, rows * c.S);
    mem.scratch(&dwork, static_cast<size_t>(B > 0 ? adr_scenario_subbook_work(n, B, c.S) : adr_credit_scenario_pv_work(n, c.S)));
    const hipError_t e = mem.begin(stream);
    Curves dc = c;
    if (curves_on_host) { dc.times = ht; dc.dfs = hd; }
    dc.dz = ddz;
    const Extra dx{dzs, dbucket, x.n_fix, dft, x.n_flt, dlt};
    if (e == hipSuccess) rc = enqueue(w, ctx, dc, trades, dx, dpv, dbook, dwork, stream, B, dplan);
    return mem.finish(w, rc, e, stream);
}

template <bool kLog>
void host_chunks(const Curves& c, const double* tab, const HostBatch& t, const Legs& arrays, const Extra& x, double* pv,
                 double* work, int64_t lo, int64_t hi, const int64_t* bounds = nullptr) {
    const int S = c.S, K = c.K;
    const size_t ds = c.S_disc == 1 ? 0 : K, zs = c.S_spr == 1 ? 0 : c.G;
    std::vector<Acc> acc(static_cast<size_t>(S));
    std::vector<double> book(static_cast<size_t>(S)), xs(static_cast<size_t>(S));
    const bool weighted = arrays.flt_weight != nullptr;
    for (int64_t ch = lo; ch < hi; ++ch) {
        std::fill(book.begin(), book.end(), 0.0);
        const ChunkRange r = host_chunk_range(ch, bounds, t.n);
        for (int64_t i = r.i0; i < r.i1; ++i) {
            Legs g = arrays;
            g.f0 = t.fix_off[i]; g.l0 = t.flt_off[i];
            g.n_fix = static_cast<int>(t.fix_off[i + 1] - t.fix_off[i]);
            g.n_flt = static_cast<int>(t.flt_off[i + 1] - t.flt_off[i]);
            g.spread = t.spread[i];
            const double z = x.z[i];
            const int bucket = x.bucket[i];
            const bool spread_on = !(z == 0.0 && bucket == -1);
            for (int s = 0; s < S; ++s) xs[s] = z + (bucket >= 0 ? c.dz[static_cast<size_t>(s) * zs + bucket] : 0.0);
            std::fill(acc.begin(), acc.end(), Acc{0.0, 0.0, 0.0});
            for (int j = 0; j < std::max(g.n_fix, g.n_flt); ++j) {
                const Slot slot = make_slot<kLog>(g, j, spread_on, c.times, K, c.method);
                if (spread_on)
                    for (int s = 0; s < S; ++s)
                        apply_slot<kLog, true>(slot, weighted, HostTab{tab + static_cast<size_t>(s) * ds}, xs[s], acc[s]);
                else
                    for (int s = 0; s < S; ++s)
                        apply_slot<kLog, false>(slot, weighted, HostTab{tab + static_cast<size_t>(s) * ds}, 0.0, acc[s]);
            }
            for (int s = 0; s < S; ++s) {
                const double v = trade_pv(acc[s], t.fix_sign[i], t.flt_sign[i], t.notional[i]);
                if (pv) pv[i * S + s] = v;
                book[s] = book[s] + v;
            }
        }
        std::copy(book.begin(), book.end(), work + ch * S);
    }
}

}  // namespace cscen
}  // namespace adr

namespace CS = adr::cscen;

extern "C" {

int64_t adr_credit_scenario_pv_work(int64_t n, int S) { return adr_scenario_pv_work(n, S); }     // the same chunks

int adr_credit_scenario_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S_disc, const double* dfs_dev,
                               int G, int S_spr, const double* dz_dev, int S, const adr_trades* trades, const double* z_dev,
                               const int32_t* bucket_dev, int64_t n_fix, const double* fix_tau_dev, int64_t n_flt,
                               const double* flt_tau_dev, double* pv_dev, double* book_pv_dev, double* work_dev, void* stream) {
    const CS::Curves c{interp_method, K, times_dev, S_disc, dfs_dev, G, S_spr, dz_dev, S};
    const CS::Extra x{z_dev, bucket_dev, n_fix, fix_tau_dev, n_flt, flt_tau_dev};
    return CS::enqueue("adr_credit_scenario_pv_dev", ctx, c, trades, x, pv_dev, book_pv_dev, work_dev, static_cast<hipStream_t>(stream));
}

int adr_credit_scenario_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S_disc, const double* dfs, int G,
                           int S_spr, const double* dz, int S, const adr_trades* trades, const double* z, const int32_t* bucket,
                           int64_t n_fix, const double* fix_tau, int64_t n_flt, const double* flt_tau, double* pv,
                           double* book_pv) {
    const CS::Curves c{interp_method, K, times, S_disc, dfs, G, S_spr, dz, S};
    const CS::Extra x{z, bucket, n_fix, fix_tau, n_flt, flt_tau};
    return CS::run_blocking("adr_credit_scenario_pv", ctx, c, true, trades, x, pv, book_pv);
}

int adr_credit_scenario_pv_set(adr_ctx* ctx, const adr_curve_set* set, int G, int S_spr, const double* dz,
                               const adr_trades* trades, const double* z, const int32_t* bucket, int64_t n_fix,
                               const double* fix_tau, int64_t n_flt, const double* flt_tau, double* pv, double* book_pv) {
    const std::string w = "adr_credit_scenario_pv_set";
    CS::SetCurves v;                                        // adr_curve_set_arrays' arrays
    const int rc = CS::curve_set_curves(w, ctx, set, &v);
    if (rc != ADR_OK) return rc;
    const CS::Curves c{v.method, v.K, v.times, v.S, v.dfs, G, S_spr, dz, v.S};
    const CS::Extra x{z, bucket, n_fix, fix_tau, n_flt, flt_tau};
    return CS::run_blocking(w, ctx, c, false, trades, x, pv, book_pv);
}

// The host entries' body; B > 0: book_pv is sub_pv[B][S] of the sub-books sub_off.
static int credit_host_run(const std::string& w, const CS::Curves& c, const CS::HostBatch& t, const double* z, const int32_t* bucket,
                           const double* fix_tau, const double* flt_tau, double* pv, double* book_pv, int n_threads, int64_t B,
                           const int64_t* sub_off) {
    const int64_t n = t.n;
    if (!t.fix_off || !t.flt_off || !t.notional || !t.spread || !t.fix_sign || !t.flt_sign)
        return adr_set_error(ADR_ERR_INVALID, w + ": null per-trade array");
    if (n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one trade is needed");
    int rc = CS::check_leg_offsets(w, t, 0, n);
    if (rc != ADR_OK) return rc;
    const CS::Extra x{z, bucket, t.fix_off[n], fix_tau, t.flt_off[n], flt_tau};
    rc = CS::validate(w, c, n, x, book_pv);
    if (rc == ADR_OK) rc = CS::check_curves(w, c.K, c.times, c.S_disc, c.dfs, "row");
    if (rc == ADR_OK) rc = CS::check_spreads(w, c, n, x);
    if (rc == ADR_OK) rc = CS::check_trade_values(w, t, 0, n);
    if (rc == ADR_OK) rc = CS::check_flows(w, t);
    if (rc != ADR_OK) return rc;
    const int S = c.S;
    const bool lin = c.method == ADR_INTERP_LINEAR_FWD_RATES;
    std::vector<double> tab(c.dfs, c.dfs + static_cast<size_t>(c.S_disc) * c.K);
    if (!lin)
        for (double& v : tab) v = std::log(v);
    std::vector<int64_t> plan;
    if (B > 0) {
        rc = adr::sub::build_plan(w, n, B, sub_off, plan);
        if (rc != ADR_OK) return rc;
    }
    const int64_t* bounds = B > 0 ? plan.data() + B + 1 : nullptr;
    const int64_t chunks = B > 0 ? plan[B] : (n + CS::kChunk - 1) / CS::kChunk;
    std::vector<double> work(static_cast<size_t>(chunks) * S);
    const CS::Legs arrays{t.fix_tp, t.fix_pay, t.flt_tp, t.flt_ts, t.flt_te, t.flt_alpha, t.flt_weight, fix_tau, flt_tau, 0, 0, 0, 0, 0.0};
    const int threads = n_threads > 0 ? static_cast<int>(std::min<int64_t>(n_threads, chunks)) : adr::pool_threads(chunks, 4);
    adr::parallel_ranges(chunks, threads, [&](int, int64_t lo, int64_t hi) {
        if (lin) CS::host_chunks<false>(c, tab.data(), t, arrays, x, pv, work.data(), lo, hi, bounds);
        else CS::host_chunks<true>(c, tab.data(), t, arrays, x, pv, work.data(), lo, hi, bounds);
    });
    if (B > 0) adr::sub::reduce_subbooks(work.data(), plan.data(), B, S, book_pv);
    else CS::reduce_chunks(work.data(), chunks, S, book_pv);
    return ADR_OK;
}

int adr_credit_scenario_pv_host(int interp_method, int K, const double* times, int S_disc, const double* dfs, int G, int S_spr,
                                const double* dz, int S, int64_t n, const int64_t* fix_off, const int64_t* flt_off,
                                const double* fix_tp, const double* fix_pay, const double* flt_tp, const double* flt_ts,
                                const double* flt_te, const double* flt_alpha, const double* flt_weight, const double* notional,
                                const double* spread, const double* fix_sign, const double* flt_sign, const double* z,
                                const int32_t* bucket, const double* fix_tau, const double* flt_tau, double* pv, double* book_pv,
                                int n_threads) {
    const CS::Curves c{interp_method, K, times, S_disc, dfs, G, S_spr, dz, S};
    const CS::HostBatch t{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional, spread,
                          fix_sign, flt_sign};
    return credit_host_run("adr_credit_scenario_pv_host", c, t, z, bucket, fix_tau, flt_tau, pv, book_pv, n_threads, 0, nullptr);
}

int adr_credit_scenario_subbook_pv_host(int interp_method, int K, const double* times, int S_disc, const double* dfs, int G,
                                        int S_spr, const double* dz, int S, int64_t n, const int64_t* fix_off,
                                        const int64_t* flt_off, const double* fix_tp, const double* fix_pay, const double* flt_tp,
                                        const double* flt_ts, const double* flt_te, const double* flt_alpha,
                                        const double* flt_weight, const double* notional, const double* spread,
                                        const double* fix_sign, const double* flt_sign, const double* z, const int32_t* bucket,
                                        const double* fix_tau, const double* flt_tau, int64_t B, const int64_t* sub_off,
                                        double* pv, double* sub_pv, int n_threads) {
    const std::string w = "adr_credit_scenario_subbook_pv_host";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const CS::Curves c{interp_method, K, times, S_disc, dfs, G, S_spr, dz, S};
    const CS::HostBatch t{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional, spread,
                          fix_sign, flt_sign};
    return credit_host_run(w, c, t, z, bucket, fix_tau, flt_tau, pv, sub_pv, n_threads, B, sub_off);
}

int adr_credit_scenario_subbook_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S_disc, const double* dfs,
                                   int G, int S_spr, const double* dz, int S, const adr_trades* trades, const double* z,
                                   const int32_t* bucket, int64_t n_fix, const double* fix_tau, int64_t n_flt,
                                   const double* flt_tau, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv) {
    const std::string w = "adr_credit_scenario_subbook_pv";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const CS::Curves c{interp_method, K, times, S_disc, dfs, G, S_spr, dz, S};
    const CS::Extra x{z, bucket, n_fix, fix_tau, n_flt, flt_tau};
    return CS::run_blocking(w, ctx, c, true, trades, x, pv, sub_pv, B, sub_off);
}

int adr_credit_scenario_subbook_pv_set(adr_ctx* ctx, const adr_curve_set* set, int G, int S_spr, const double* dz,
                                       const adr_trades* trades, const double* z, const int32_t* bucket, int64_t n_fix,
                                       const double* fix_tau, int64_t n_flt, const double* flt_tau, int64_t B,
                                       const int64_t* sub_off, double* pv, double* sub_pv) {
    const std::string w = "adr_credit_scenario_subbook_pv_set";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    CS::SetCurves v;
    const int rc = CS::curve_set_curves(w, ctx, set, &v);
    if (rc != ADR_OK) return rc;
    const CS::Curves c{v.method, v.K, v.times, v.S, v.dfs, G, S_spr, dz, v.S};
    const CS::Extra x{z, bucket, n_fix, fix_tau, n_flt, flt_tau};
    return CS::run_blocking(w, ctx, c, false, trades, x, pv, sub_pv, B, sub_off);
}

int adr_credit_scenario_subbook_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S_disc,
                                       const double* dfs_dev, int G, int S_spr, const double* dz_dev, int S,
                                       const adr_trades* trades, const double* z_dev, const int32_t* bucket_dev, int64_t n_fix,
                                       const double* fix_tau_dev, int64_t n_flt, const double* flt_tau_dev, int64_t B,
                                       const int64_t* plan_dev, double* pv_dev, double* sub_pv_dev, double* work_dev, void* stream) {
    const std::string w = "adr_credit_scenario_subbook_pv_dev";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const CS::Curves c{interp_method, K, times_dev, S_disc, dfs_dev, G, S_spr, dz_dev, S};
    const CS::Extra x{z_dev, bucket_dev, n_fix, fix_tau_dev, n_flt, flt_tau_dev};
    return CS::enqueue(w, ctx, c, trades, x, pv_dev, sub_pv_dev, work_dev, static_cast<hipStream_t>(stream), B, plan_dev);
}

}  // extern "C"
