// The per-coupon code of a TradeBatch under scenario curves, shared by scenario_pv.hip (one curve per scenario) and
// xccy_scenario_pv.hip (two: forwards from one table, discount factors from another): the coupon description (Slot), how
// a lane forms it, how it travels to the wave's scalar registers, how a scenario evaluates it, the trade's PV, and the
// host twins' chunk walk and batch checks.  The host twins and the device are held to this code bit for bit.
//
// A coupon reads its accrual dates ts, te on the FORWARD grid and its payment date tp - like every fixed flow - on the
// DISCOUNT grid.  kTwo = false: the two grids are one (scenario_pv.hip), so a payment on the accrual end takes the D(te)
// just computed (kTpIsTe).  kTwo = true: they differ, D(tp) is always looked up on the discount table; on equal tables
// that lookup has D(te)'s bits, so the two forms agree bit for bit there.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "host_pool.hpp"
#include "scenario_common.hpp"
#include "subbook.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace scen {

// Coupon index c of a trade: its float coupon (c < n_flt) and its fixed flow (c < n_fix).  The masks are adr_price's
// (the reference engine's): a float coupon counts when tp >= 0 and has no forward when alpha <= 0, a fixed flow counts
// when tp > 0.
enum : int {
    kHasFlt = 1, kHasFix = 2,
    kTsIsPrevTe = 4,     // accrual start == the previous coupon's accrual end: D(ts) is the D(te) just computed
    kTpIsTe = 8,         // no payment lag, one grid: D(tp) is D(te)
    kFixIsFltTp = 16,    // the fixed flow is paid with the float coupon: D is D(tp)
    kNoAccrual = 32      // alpha <= 0: the coupon is spread * alpha * D(tp)
};

struct Slot {
    int flags;
    DateW ws, we, wp, wx;
    double sa, w, pay;   // spread * alpha, the coupon's notional multiplier, the fixed amount
};

struct Legs {            // one trade's cash flows
    const double *fix_tp, *fix_pay, *flt_tp, *flt_ts, *flt_te, *flt_alpha, *flt_weight;
    int64_t f0, l0;
    int n_fix, n_flt;
    double spread;
};

struct Grid {            // what a description needs of a curve: the knots, not the values
    const double* x;
    int K, method;
};

template <bool kLog, bool kTwo>
__host__ __device__ inline Slot make_slot(const Legs& g, int c, const Grid& fwd, const Grid& dsc) {
    Slot s;
    s.flags = 0;
    s.ws = s.we = s.wp = s.wx = DateW{0, 0, 0.0, 0.0};
    s.sa = 0.0; s.w = 1.0; s.pay = 0.0;
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
        if (al > 0.0) {
            // the previous coupon left its D(te) behind when it counted and accrued
            if (c > 0 && ts == g.flt_te[i - 1] && g.flt_tp[i - 1] >= 0.0 && g.flt_alpha[i - 1] > 0.0) s.flags |= kTsIsPrevTe;
            else s.ws = date_weights<kLog>(ts, fwd.x, fwd.K, fwd.method);
            s.we = date_weights<kLog>(te, fwd.x, fwd.K, fwd.method);
            if (!kTwo && tp == te) s.flags |= kTpIsTe;
            else s.wp = date_weights<kLog>(tp, dsc.x, dsc.K, dsc.method);
        } else {
            s.flags |= kNoAccrual;
            s.wp = date_weights<kLog>(tp, dsc.x, dsc.K, dsc.method);
        }
    }
    if (c < g.n_fix) {
        const int64_t i = g.f0 + c;
        const double xt = g.fix_tp[i];
        if (xt > 0.0) {
            s.flags |= kHasFix;
            s.pay = g.fix_pay[i];
            if (flt && xt == tp) s.flags |= kFixIsFltTp;
            else s.wx = date_weights<kLog>(xt, dsc.x, dsc.K, dsc.method);
        }
    }
    return s;
}

struct Acc {             // one scenario's running state inside a trade
    double de, flt, fix; // D(te) of the previous coupon; the legs' sums before sign and notional
};

// ftab: the scenario's forward table; dtab: its discount table (the same object in scenario_pv.hip).
template <bool kLog, class FTab, class DTab>
__host__ __device__ inline void apply_slot(const Slot& s, bool weighted, const FTab& ftab, const DTab& dtab, Acc& a) {
    double dp = 0.0;
    if (s.flags & kHasFlt) {
        double term;
        if (s.flags & kNoAccrual) {
            dp = eval_df<kLog>(s.wp, dtab);
            term = s.sa * dp;
        } else {
            const double ds = (s.flags & kTsIsPrevTe) ? a.de : eval_df<kLog>(s.ws, ftab);
            const double de = eval_df<kLog>(s.we, ftab);
            dp = (s.flags & kTpIsTe) ? de : eval_df<kLog>(s.wp, dtab);
            term = ((ds / de - 1.0) + s.sa) * dp;
            a.de = de;
        }
        if (weighted) term = s.w * term;
        a.flt = a.flt + term;
    }
    if (s.flags & kHasFix) {
        const double dx = (s.flags & kFixIsFltTp) ? dp : eval_df<kLog>(s.wx, dtab);
        a.fix = a.fix + s.pay * dx;
    }
}

// + 0.0: a trade without a live flow has two zero sums, and with fix_sign = -1 and flt_sign * notional < 0 both products are
// -0.0; the PV of nothing is +0.0.  Every other value passes through the add unchanged.
__host__ __device__ inline double trade_pv(const Acc& a, double fix_sign, double flt_sign, double notional) {
    return (fix_sign * a.fix + (flt_sign * notional) * a.flt) + 0.0;
}

// Lane j's slot in scalar registers; only the parts its flags say will be read.
__device__ inline Slot lane_slot(const Slot& m, int j, bool weighted) {
    Slot u;
    u.flags = lane_int(m.flags, j);
    u.ws = u.we = u.wp = u.wx = DateW{0, 0, 0.0, 0.0};
    u.sa = 0.0; u.w = 1.0; u.pay = 0.0;
    if (u.flags & kHasFlt) {
        if (!(u.flags & kNoAccrual)) {
            if (!(u.flags & kTsIsPrevTe)) u.ws = lane_date(m.ws, j);
            u.we = lane_date(m.we, j);
        }
        if (!(u.flags & kTpIsTe)) u.wp = lane_date(m.wp, j);
        u.sa = lane_dbl(m.sa, j);
        if (weighted) u.w = lane_dbl(m.w, j);
    }
    if (u.flags & kHasFix) {
        if (!(u.flags & kFixIsFltTp)) u.wx = lane_date(m.wx, j);
        u.pay = lane_dbl(m.pay, j);
    }
    return u;
}

// -------------------------------------------------------------------------------------------------------------- host
// The chunks lo .. hi - 1 of a host twin: ftab / dtab are the converted tables, row s at s * stride (0: a shared row).
template <bool kLog, bool kTwo>
void host_chunks(const Grid& fwd, const Grid& dsc, int S, const double* ftab, size_t f_stride, const double* dtab, size_t d_stride,
                 const HostBatch& t, const Legs& arrays, double* pv, double* work, int64_t lo, int64_t hi,
                 const int64_t* bounds = nullptr) {
    std::vector<Acc> acc(static_cast<size_t>(S));
    std::vector<double> book(static_cast<size_t>(S));
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
            std::fill(acc.begin(), acc.end(), Acc{0.0, 0.0, 0.0});
            for (int c = 0; c < std::max(g.n_fix, g.n_flt); ++c) {
                const Slot slot = make_slot<kLog, kTwo>(g, c, fwd, dsc);
                for (int s = 0; s < S; ++s)
                    apply_slot<kLog>(slot, weighted, HostTab{ftab + static_cast<size_t>(s) * f_stride},
                                     HostTab{dtab + static_cast<size_t>(s) * d_stride}, acc[s]);
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

// What a _host entry can read of its batch; trade by trade, so the first trade at fault decides the message.
inline int check_host_batch(const std::string& w, const HostBatch& t) {
    if (!t.fix_off || !t.flt_off || !t.notional || !t.spread || !t.fix_sign || !t.flt_sign)
        return adr_set_error(ADR_ERR_INVALID, w + ": null per-trade array");
    int rc = ADR_OK;
    for (int64_t i = 0; rc == ADR_OK && i < t.n; ++i) {
        rc = check_leg_offsets(w, t, i, i + 1);
        if (rc == ADR_OK) rc = check_trade_values(w, t, i, i + 1);
    }
    if (rc == ADR_OK) rc = check_flows(w, t);
    return rc;
}

// A host twin's body once its inputs are checked: the tables converted once (ln d under the log schemes), the chunks
// on CPU threads, then the book sum, or with B > 0 the sums of the sub-books sub_off into book[B][S].  rows_f / rows_d:
// 1 (a shared row) or S.  kTwo = false: the discount arguments repeat the forward ones and one table serves both.
template <bool kTwo>
int host_book_run(const std::string& w, const Grid& fwd, int rows_f, const double* fdfs, const Grid& dsc, int rows_d,
                  const double* ddfs, int S, const HostBatch& t, double* pv, double* book, int n_threads, int64_t B,
                  const int64_t* sub_off) {
    const bool lin = fwd.method == ADR_INTERP_LINEAR_FWD_RATES;
    auto table = [lin](const double* dfs, int rows, int K) {
        std::vector<double> tab(dfs, dfs + static_cast<size_t>(rows) * K);
        if (!lin)
            for (double& v : tab) v = std::log(v);
        return tab;
    };
    const std::vector<double> ftab = table(fdfs, rows_f, fwd.K);
    const std::vector<double> dtab_own = kTwo ? table(ddfs, rows_d, dsc.K) : std::vector<double>();
    const double* dtab = kTwo ? dtab_own.data() : ftab.data();
    const size_t fs = rows_f == 1 ? 0 : fwd.K, ds = rows_d == 1 ? 0 : dsc.K;
    std::vector<int64_t> plan;
    if (B > 0) {
        const int rc = sub::build_plan(w, t.n, B, sub_off, plan);
        if (rc != ADR_OK) return rc;
    }
    const int64_t* bounds = B > 0 ? plan.data() + B + 1 : nullptr;
    const int64_t chunks = B > 0 ? plan[B] : (t.n + kChunk - 1) / kChunk;
    std::vector<double> work(static_cast<size_t>(chunks) * S);
    const Legs arrays{t.fix_tp, t.fix_pay, t.flt_tp, t.flt_ts, t.flt_te, t.flt_alpha, t.flt_weight, 0, 0, 0, 0, 0.0};
    const int threads = std::max(1, n_threads > 0 ? static_cast<int>(std::min<int64_t>(n_threads, chunks)) : adr::pool_threads(chunks, 4));
    adr::parallel_ranges(chunks, threads, [&](int, int64_t lo, int64_t hi) {
        if (lin) host_chunks<false, kTwo>(fwd, dsc, S, ftab.data(), fs, dtab, ds, t, arrays, pv, work.data(), lo, hi, bounds);
        else host_chunks<true, kTwo>(fwd, dsc, S, ftab.data(), fs, dtab, ds, t, arrays, pv, work.data(), lo, hi, bounds);
    });
    if (B > 0) sub::reduce_subbooks(work.data(), plan.data(), B, S, book);
    else reduce_chunks(work.data(), chunks, S, book);
    return ADR_OK;
}

}  // namespace scen
}  // namespace adr
