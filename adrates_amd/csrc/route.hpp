// Launch plan of a pricing call: which kernel family takes which set of trades, on what grid, and where its block partials
// go.  Pure host logic (no HIP call): adr_price_dev builds the plan from the curve's class and the batch's table sizes and
// replays it; adr_route_host runs the same three functions (curve_class, trade_layout, make_plan) for a CPU test that
// checks, over the cross product of trade classes, curve classes, schemes and requests, that every trade is priced
// exactly once (tests/test_route_table.py).
//
// The reference has one route - Engine._compute_ois_natural walks a trade's legs whatever they look like
// (cavour/market/position/engine.py:153-215); everything here is about which specialised kernel gives the same numbers fastest.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "kernels.hpp"

namespace adr {
namespace route {

// kernel families
enum Family : int {
    F_LITE = 0,           // lite kernel: PV / PV + delta, 16-slot rows, trades without payment lag (<= 384 coupons per leg)
    F_LITE_LAG = 1,       // ... its payment-lag rows (<= 360 coupons, log-linear schemes)
    F_FAST = 2,           // fast kernel on the 32-slot row table
    F_FAST_CHAINED = 3,   // ... chains of rows (33-384 coupons per leg)
    F_FAST_LAG = 4,       // payment-lag variant of the fast kernel, one-row trades (GAMMA, packed layout, log-linear, even P)
    F_FAST_LAG_CHAINED = 5,   // ... chains of rows (33-128 coupons)
    F_GENERAL = 6,        // general kernel over a trade list
    F_WIDE = 7,           // wide variants of the general kernel (33-64 pillars, one launch)
    F_TILED = 8,          // general kernel once per pair of 32-pillar tiles (curves whose wide tables do not fit / PILLAR_TILES)
    F_KNOT = 9,           // aggregate-only: knot-space sums of the lite table's trades + one projection
    F_KNOT_LAG = 10       // ... of the lite kernel's payment-lag rows (ratio nodes: pair bands; log-linear schemes)
};
// trade sets (adr_trades: tables and lists built by adr_trades_upload)
enum Set : int {
    S_LITE = 0, S_LITE_LAG = 1, S_ROWS = 2, S_CHAINED = 3, S_LAGGED = 4, S_LAGGED_CHAINED = 5,
    S_GENERAL = 6,        // payment lag / weights, or more than 384 coupons per leg
    S_GENERAL_B = 7,      // ... without the trades of the lite kernel's payment-lag rows
    S_REST = 8,           // ... without the trades of the payment-lag variant's tables
    S_NONLITE = 9,        // every trade outside the lite table
    S_NONLITE_B = 10,     // ... and outside the lite kernel's payment-lag rows
    S_ALL = 11
};
constexpr int kSets = S_ALL + 1;

struct Launch {
    int family, set;
    int64_t items;        // rows / units / list entries the launch covers
    int blocks;
    int first_block;      // where its block partials start (in blocks of the plan's partial stride)
    int tile_i, tile_j;   // F_TILED only
};

// sizes of a batch's tables and lists (adr_trades), all the plan needs to know about the trades
struct TradeCounts {
    int64_t n = 0;
    int64_t rows = 0, chained_rows = 0, lagged_rows = 0, lagged_chained_rows = 0;
    int64_t lite_units = 0, lite_lag_units = 0;
    int64_t n_general = 0, n_general_b = 0, n_rest = 0, n_nonlite = 0, n_nonlite_b = 0;
    int chained_blocks = 0, lagged_chained_blocks = 0, lag_blocks = 0;
    bool lag_scratch = false;
};

struct Plan {
    std::vector<Launch> launches;    // in launch order; F_KNOT (if any) last: it ADDS to the aggregate the others' reduction wrote
    int total_blocks = 0;            // blocks that write partials (all families but F_KNOT, F_TILED keeps its own layout)
    bool wide = false;               // partials in the wide layout (launch_reduce_wide)
    bool tiled = false;              // one reduction per tile launch
    bool knot = false, knot_lag = false;
    const char* error = nullptr;     // "grid exceeds scratch"
};

constexpr size_t kLds = 160 * 1024;
constexpr int kKnotMaxKc = 640;             // reachable knots a curve can have for the knot pass (its dense 32-wide Jacobian must fit the LDS)
constexpr int kKnotLagMaxKc = 256;          // ... for the knot pass over payment-lag rows (16 pair bands per knot, a dense overflow matrix)

// The scratch grids of a device of n_cu CUs (adr_ctx): block partials for max_blocks blocks, knot-pass records for knot_blocks
struct Grid { int max_blocks, knot_blocks; };
inline Grid grid_for(int n_cu) {
    const int cu = std::max(1, n_cu);
    return Grid{cu * 16, cu * kLiteWavesPerSimd * 4 * 64 / kLiteThreads};     // (knot pass: the blocks resident at once)
}

// The class of a curve: everything about it the plan reads.  Two curves of one class get the same plan, so the class plus
// the request is the key of the plan a batch caches.
struct CurveClass {
    int K, Kc, P, T, method;
    int wide_nch;       // chunks of the wide layout's tables when the curve takes the wide route, else 0
    int packed_ok;      // the packed layout exists and the fast kernel's tables fit the LDS
    int lds_rows;       // GAMMA: the general kernel's variant with LDS-resident convexity rows serves the curve
    int n_lut, Kcore, pc_pad, Ec, epg, cpg, n_mini;    // what the kernels' LDS sizes read besides (kernels.hpp)
    CurveDev sizes() const {                           // a CurveDev without tables, for those size functions
        CurveDev d{};
        d.K = K; d.Kc = Kc; d.P = P; d.T = T; d.method = method; d.wide_nch = wide_nch; d.packed_ok = packed_ok;
        d.n_lut = n_lut; d.Kcore = Kcore; d.pc_pad = pc_pad; d.Ec = Ec; d.epg = epg; d.cpg = cpg; d.n_mini = n_mini;
        return d;
    }
};

// The class of the curve of tables t under interpolation scheme `method`; pillar_tiles: ADR_CURVE_PILLAR_TILES.
// 33-64 pillars take the wide route when its tables fit the LDS, else the tiles; the packed layout of up to 32 pillars serves
// the fast kernels only when their tables fit the LDS next to the search arrays, else the general kernel serves all.
inline CurveClass curve_class(const CurveTables& t, int method, bool pillar_tiles) {
    CurveClass c{};
    c.K = t.K; c.Kc = t.Kc; c.P = t.P; c.T = t.T; c.method = method;
    c.n_lut = static_cast<int>(t.lut.size() / 2); c.Kcore = t.Kcore; c.pc_pad = t.pc_pad; c.Ec = t.Ec; c.epg = t.epg; c.cpg = t.cpg;
    c.n_mini = t.n_mini;
    const bool wide = t.wide_nch > 0 && t.wide_nch <= kWideMaxChunks && !pillar_tiles &&
                      wide_kernel_lds_bytes(t.K, t.Kc, t.wide_nch, t.has_hess) <= kLds;
    c.wide_nch = wide ? t.wide_nch : 0;
    c.packed_ok = t.packed_ok && fast_kernel_lds_bytes(c.sizes(), t.has_hess) <= kLds ? 1 : 0;
    // (the convexity rows are uploaded with the packed layout, whether or not the fast kernel's tables fit)
    c.lds_rows = t.has_hess && t.packed_ok && t.T == 1 &&
                 general_lds_rows_fit(general_lds_kernel_lds_bytes_for(t.K, t.Kc, t.Kcore, t.Ec, t.n_mini, c.n_lut, true), t.Ec, t.n_fringe);
    return c;
}

inline int blocks_for(int64_t units, int waves, int64_t cap) {
    const int64_t need = (units + waves - 1) / waves;
    return static_cast<int>(std::min<int64_t>(need, cap));
}

// per_trade: some per-trade output pointer is non-null; has_agg: agg is requested.
inline Plan make_plan(const CurveClass& cc, const TradeCounts& tc, bool want_delta, bool want_gamma, bool per_trade, bool has_agg,
                      int n_cu) {
    Plan plan;
    const int64_t n = tc.n;
    if (n == 0) return plan;
    const CurveDev cv = cc.sizes();
    const int max_blocks = grid_for(n_cu).max_blocks, knot_blocks = grid_for(n_cu).knot_blocks;
    const bool lite_fits = lite_kernel_lds_bytes(cv, want_delta, true) <= kLds;
    const bool log_linear = cv.method != 2;
    // aggregate-only request: the lite table's trades in knot space
    plan.knot = has_agg && !per_trade && want_delta && tc.lite_units > 0 && cv.Kc <= kKnotMaxKc &&
                knot_kernel_lds_bytes(cv, want_gamma) <= kLds;
    // ... and the payment-lag rows' (ratio nodes, any scheme; the pair bands of 16 want more LDS and scratch per knot)
    plan.knot_lag = has_agg && !per_trade && want_delta && tc.lite_lag_units > 0 && cv.Kc <= kKnotLagMaxKc &&
                    (plan.knot || tc.lite_units == 0) && knot_kernel_lds_bytes(cv, want_gamma, true) <= kLds;
    // the trades no knot pass takes: everything / outside the lite table / and outside its payment-lag rows
    const int rest_of_knot = plan.knot_lag ? S_NONLITE_B : (plan.knot ? S_NONLITE : S_ALL);
    const int64_t rest_of_knot_n = plan.knot_lag ? tc.n_nonlite_b : (plan.knot ? tc.n_nonlite : n);
    auto lite_blocks = [&](int64_t units, bool lag = false) {
        const size_t lds = lite_kernel_lds_bytes(cv, want_delta, lag);
        const int threads = lite_kernel_threads(cv, want_delta, lag);
        // (blocks of more than 512 threads are built for ONE per CU: their registers allow no second)
        const int per_cu = threads > kLiteThreads ? 1 : static_cast<int>(std::max<size_t>(1, std::min<size_t>(2, kLds / lds)));
        return blocks_for(units, threads / 64, static_cast<int64_t>(n_cu) * per_cu);
    };
    auto push = [&](int family, int set, int64_t items, int blocks, int ti = 0, int tj = 0) {
        if (items <= 0 || blocks <= 0) return;
        plan.launches.push_back(Launch{family, set, items, blocks, plan.total_blocks, ti, tj});
        if (family != F_KNOT) plan.total_blocks += blocks;
    };
    auto knot_launch = [&]() {
        for (int lag = 0; lag < 2; ++lag) {
            if (!(lag ? plan.knot_lag : plan.knot)) continue;
            const size_t lds = knot_kernel_lds_bytes(cv, want_gamma, lag != 0);
            const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(2, kLds / lds)));
            const int64_t units = lag ? tc.lite_lag_units : tc.lite_units;
            const int blocks = blocks_for(units, knot_kernel_threads() / 64, std::min<int64_t>(static_cast<int64_t>(n_cu) * per_cu, knot_blocks));
            plan.launches.push_back(Launch{lag ? F_KNOT_LAG : F_KNOT, lag ? S_LITE_LAG : S_LITE, units, blocks, 0, 0, 0});
        }
    };

    if (cv.T > 1 && cv.wide_nch > 0) {
        // 33-64 pillars, one launch for the whole ladder.  GAMMA: the wide variants; PV / PV + delta: the lite kernel's 64-pillar
        // instantiations for the trades of its tables, the wide kernel for the rest.
        plan.wide = true;
        const bool lite_elsewhere = (!want_gamma && lite_fits && tc.lite_units > 0) || plan.knot;
        const bool use_lite_lag = (!want_gamma && lite_fits && tc.lite_lag_units > 0) || plan.knot_lag;   // (priced elsewhere)
        int rest_set = S_ALL;
        int64_t rest_n = n;
        if (lite_elsewhere || use_lite_lag) {     // (no plain lite rows means no trade is outside list_nonlite)
            rest_set = use_lite_lag ? S_NONLITE_B : S_NONLITE;
            rest_n = use_lite_lag ? tc.n_nonlite_b : tc.n_nonlite;
        }
        if (lite_elsewhere && !plan.knot) push(F_LITE, S_LITE, tc.lite_units, lite_blocks(tc.lite_units));
        if (use_lite_lag && !plan.knot_lag) push(F_LITE_LAG, S_LITE_LAG, tc.lite_lag_units, lite_blocks(tc.lite_lag_units, true));
        if (rest_n > 0) {
            const size_t lds = wide_kernel_lds_bytes(cv.K, cv.Kc, cv.wide_nch, want_gamma);
            const int threads = wide_kernel_threads(cv.wide_nch, want_gamma);
            push(F_WIDE, rest_set, rest_n, blocks_for(rest_n, threads / 64, static_cast<int64_t>(n_cu) * wide_kernel_blocks_per_cu(lds, threads)));
        }
        if (static_cast<size_t>(plan.total_blocks) * wide_partial_doubles(cv.wide_nch) > static_cast<size_t>(max_blocks) * kAggStride)
            plan.error = "grid exceeds scratch";
        knot_launch();
        return plan;
    }
    if (cv.T > 1) {
        // ... or once per pair of pillar tiles (tile_i <= tile_j): each launch writes its tile of the ladders
        plan.tiled = true;
        const int T = cv.T;
        const int set = rest_of_knot;
        const int64_t items = rest_of_knot_n;
        const int blocks = blocks_for(items, kGeneralThreads / 64, static_cast<int64_t>(n_cu) * 4);
        for (int tj = 0; tj < T; ++tj)
            for (int ti = 0; ti <= tj; ++ti) {
                if (!want_gamma && ti != tj) continue;               // PV / delta live on the diagonal tiles
                if (!want_delta && tj > 0) continue;                 // PV alone: tile (0, 0) has it
                push(F_TILED, set, items, blocks, ti, tj);
            }
        // (every tile launch is followed by its own reduction: the launches of a pass share one range of the scratch)
        for (Launch& L : plan.launches) L.first_block = 0;
        plan.total_blocks = plan.launches.empty() ? 0 : blocks;
        if (plan.total_blocks > max_blocks) plan.error = "grid exceeds scratch";
        knot_launch();
        return plan;
    }

    // Up to 32 pillars.  With GAMMA: trades without payment lag take the fast kernel when the curve has the packed layout
    // (more than 32 coupons per leg: chains of rows), payment-lag / weighted trades its payment-lag variant (log-linear
    // schemes, even pillar count), the general kernel what is left.  Without GAMMA: the lite kernel takes the trades of its
    // two tables, the chained fast kernel (packed layout) or the general kernel the rest.
    const bool use_fast = cv.packed_ok != 0;
    const bool use_lite = !want_gamma && lite_fits && tc.lite_units > 0;
    const bool lite_elsewhere = use_lite || plan.knot;
    const bool use_lite_lag = (!want_gamma && lite_fits && tc.lite_lag_units > 0) || plan.knot_lag;   // (priced elsewhere)
    const bool use_lag = want_gamma && use_fast && (tc.lagged_rows > 0 || tc.lagged_chained_rows > 0) && tc.lag_scratch &&
                         log_linear && cv.P % 2 == 0 && tc.lagged_chained_blocks <= tc.lag_blocks && !plan.knot_lag;
    int64_t rows = tc.rows, chained = tc.chained_rows;
    int general_set = S_ALL;
    int64_t general_n = n;
    if (!want_gamma && (lite_elsewhere || use_lite_lag)) {
        if (lite_elsewhere) { rows = 0; chained = 0; }        // the lite table holds the trades of both 32-slot row tables
        if (use_fast) {                                       // (without lite rows: long trades keep their chained rows)
            general_set = use_lite_lag ? S_GENERAL_B : S_GENERAL;
            general_n = use_lite_lag ? tc.n_general_b : tc.n_general;
        } else {                                              // no packed layout: long trades join the general list
            rows = 0; chained = 0;
            general_set = (lite_elsewhere && !use_lite_lag) ? S_NONLITE : S_NONLITE_B;
            general_n = (lite_elsewhere && !use_lite_lag) ? tc.n_nonlite : tc.n_nonlite_b;
        }
    } else if (use_fast) {
        general_set = plan.knot_lag ? S_GENERAL_B : (use_lag ? S_REST : S_GENERAL);
        general_n = plan.knot_lag ? tc.n_general_b : (use_lag ? tc.n_rest : tc.n_general);
        if (plan.knot) { rows = 0; chained = 0; }
    } else {
        rows = 0; chained = 0;                                // the general kernel walks every trade no knot pass takes
        general_set = rest_of_knot; general_n = rest_of_knot_n;
    }
    if (use_lite && !plan.knot) push(F_LITE, S_LITE, tc.lite_units, lite_blocks(tc.lite_units));
    if (rows > 0) {
        const size_t lds = fast_kernel_lds_bytes(cv, want_gamma);
        const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(2, kLds / lds)));
        const int64_t units = (rows + fast_kernel_groups() - 1) / fast_kernel_groups();
        push(F_FAST, S_ROWS, rows, blocks_for(units, kFastThreads / 64, static_cast<int64_t>(n_cu) * per_cu));
    }
    if (chained > 0) push(F_FAST_CHAINED, S_CHAINED, chained, tc.chained_blocks);        // the chains are laid out for this grid
    if (general_n > 0) {
        const int threads = want_gamma && cc.lds_rows ? kGeneralLdsThreads : kGeneralThreads;    // (general_kernel_threads)
        push(F_GENERAL, general_set, general_n,
             blocks_for(general_n, threads / 64, static_cast<int64_t>(n_cu) * (threads == kGeneralThreads ? 4 : 2)));
    }
    if (use_lag && tc.lagged_rows > 0) {
        const int64_t units = (tc.lagged_rows + fast_kernel_groups() - 1) / fast_kernel_groups();
        push(F_FAST_LAG, S_LAGGED, tc.lagged_rows, blocks_for(units, fast_kernel_threads(true) / 64, std::min(tc.lag_blocks, n_cu)));
    }
    if (use_lite_lag && !plan.knot_lag) push(F_LITE_LAG, S_LITE_LAG, tc.lite_lag_units, lite_blocks(tc.lite_lag_units, true));
    if (use_lag && tc.lagged_chained_rows > 0) push(F_FAST_LAG_CHAINED, S_LAGGED_CHAINED, tc.lagged_chained_rows, tc.lagged_chained_blocks);
    if (plan.total_blocks > max_blocks) plan.error = "grid exceeds scratch";
    knot_launch();
    return plan;
}

// ------------------------------------------------------------------------------------------------------------------
// Trade layout: which table or list every trade of a batch lands in, and the host side of those tables (route.cpp).
// adr_trades_upload copies it to the device and gathers the tables there (trades_build.hip); adr_route_host reads it.
// ------------------------------------------------------------------------------------------------------------------
constexpr int64_t kMaxChain = 12;                                       // rows per trade in the chained table: legs of up to 384 coupons
constexpr int64_t kMaxChainLag = kLagScratchNodes / kRowSlots;          // ... payment-lag legs: 128 (the variant's per-trade stash)

struct TradeLayout {
    // The trades of each set, in table order: a list set's list; a row table's trades (one row each, sorted by coupon count;
    // the chained tables: in the order their chains were dealt); a lite table's slots (-1: an empty slot).  S_ALL: empty.
    std::vector<int32_t> trades[kSets];
    // chained tables (S_CHAINED, S_LAGGED_CHAINED): the rows dealt to the wave columns - the row's trade (-1: empty), the
    // first coupon of its piece and "the trade continues in the group's next row"
    std::vector<int32_t> chain_trade[kSets], chain_first[kSets];
    std::vector<uint8_t> chain_more[kSets];
    // lite tables (S_LITE, S_LITE_LAG): the segment header (device pointers null) and every row's slot and piece
    LiteRowsDev lite[2] = {};
    std::vector<int32_t> lite_row_slot[2];
    std::vector<uint8_t> lite_row_piece[2];
    TradeCounts counts;
    bool any_lagged = false;      // some trade has payment lag or per-coupon notionals (TradesDev::any_ratio)
    bool too_many_rows = false;   // a lite table has more than 2^32 slots: its work lists are not built
};

// lagged_of[t] for the trades t0 <= t < t1: a float coupon of trade t accrues to a date other than its payment date (payment
// lag: ratio terms), or carries a weight != 1.  (adr_trades_upload runs it inside its validation pass, one range per thread.)
inline void flag_lagged(int64_t t0, int64_t t1, const int64_t* flt_off, const double* flt_tp, const double* flt_te,
                        const double* flt_alpha, const double* flt_weight, uint8_t* lagged_of) {
    for (int64_t t = t0; t < t1; ++t) {
        bool lag = false;
        for (int64_t j = flt_off[t]; j < flt_off[t + 1] && !lag; ++j)
            lag = (flt_alpha[j] > 0.0 && flt_te[j] != flt_tp[j]) || (flt_weight && flt_weight[j] != 1.0);
        lagged_of[t] = lag ? 1 : 0;
    }
}

// The trades' classes and tables (the offsets have been validated; lagged_of: flag_lagged).  n_cu: the grid the chained
// tables are dealt for.
TradeLayout trade_layout(int64_t n, const int64_t* fix_off, const int64_t* flt_off, const uint8_t* lagged_of, int n_cu);

}  // namespace route
}  // namespace adr
