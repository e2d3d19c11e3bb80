// Trade layout of a batch (route.hpp): the host side of adr_trades_upload, also run by adr_route_host.  No HIP call.
#include <algorithm>
#include <functional>
#include <queue>
#include <utility>

#include "route.hpp"

namespace adr {
namespace route {

namespace {
const int64_t kLiteRowBuckets[kLiteSegments] = {1, 2, 3, 4, 6, 8, 12, 16, 26};   // lite rows per trade, rounded up (26 x 15 >= 384)
}

TradeLayout trade_layout(int64_t n, const int64_t* fix_off, const int64_t* flt_off, const uint8_t* lagged_of, int n_cu) {
    TradeLayout L;
    TradeCounts& tc = L.counts;
    tc.n = n;
    const int cu = std::max(1, n_cu);
    for (int64_t t = 0; t < n; ++t) if (lagged_of[t]) { L.any_lagged = true; break; }

    auto coupons_of = [&](int64_t t) { return flt_off[t + 1] - flt_off[t]; };
    auto rows_of = [&](int64_t t) {
        const int64_t m = std::max(flt_off[t + 1] - flt_off[t], fix_off[t + 1] - fix_off[t]);
        return std::max<int64_t>(1, (m + kRowSlots - 1) / kRowSlots);
    };
    auto lite_bucket = [&](int64_t t) {
        const int64_t m = std::max(flt_off[t + 1] - flt_off[t], fix_off[t + 1] - fix_off[t]);
        const int64_t rows = std::max<int64_t>(1, (m + kLiteCoupons - 1) / kLiteCoupons);
        int b = 0;
        while (b < kLiteSegments && kLiteRowBuckets[b] < rows) ++b;
        return b;
    };

    // which table or list every trade lands in.  Lite tables: plain = the trades of the 32-slot row tables, one-row and
    // chained (legs of up to 384 coupons = 26 lite rows of 15); with payment lag / weights: as many rows as the buckets allow.
    // (seg_*[k] holds bucket kLiteSegments - 1 - k: longest first)
    std::vector<int32_t>&list_fast = L.trades[S_ROWS], &list_long = L.trades[S_CHAINED], &list_general = L.trades[S_GENERAL],
                        &list_lagged = L.trades[S_LAGGED], &list_lagged_long = L.trades[S_LAGGED_CHAINED], &list_rest = L.trades[S_REST],
                        &nonlite = L.trades[S_NONLITE], &nonlite_b = L.trades[S_NONLITE_B], &general_b = L.trades[S_GENERAL_B];
    std::vector<int32_t> seg_plain[kLiteSegments], seg_lag[kLiteSegments];
    std::vector<char> lite_lag(static_cast<size_t>(n), 0);
    for (int64_t t = 0; t < n; ++t) {
        const int64_t rows = rows_of(t);
        const bool lagged = lagged_of[static_cast<size_t>(t)] != 0;
        const bool general = rows > kMaxChain || lagged;
        (general ? list_general : rows > 1 ? list_long : list_fast).push_back(static_cast<int32_t>(t));
        if (general) (rows == 1 ? list_lagged : rows <= kMaxChainLag ? list_lagged_long : list_rest).push_back(static_cast<int32_t>(t));
        const int bucket = lite_bucket(t);
        if (!general) { seg_plain[kLiteSegments - 1 - bucket].push_back(static_cast<int32_t>(t)); continue; }
        nonlite.push_back(static_cast<int32_t>(t));
        if (lagged && bucket < kLiteSegments) {
            seg_lag[kLiteSegments - 1 - bucket].push_back(static_cast<int32_t>(t));
            lite_lag[static_cast<size_t>(t)] = 1;
        } else {
            nonlite_b.push_back(static_cast<int32_t>(t));
        }
    }
    for (int32_t t : list_general) if (!lite_lag[static_cast<size_t>(t)]) general_b.push_back(t);

    // stable order by float-coupon count, longest first (the trades sharing a wavefront then have similar lengths):
    // a counting sort for the one-row tables (at most 32 coupons), std::stable_sort for the short lists of longer trades
    auto sort_by_coupons = [&](std::vector<int32_t>& list) {
        bool small = true;
        for (int32_t t : list) small &= coupons_of(t) <= 64;
        if (!small) {
            std::stable_sort(list.begin(), list.end(), [&](int32_t a, int32_t b) { return coupons_of(a) > coupons_of(b); });
            return;
        }
        size_t count[66] = {0};
        for (int32_t t : list) ++count[64 - coupons_of(t) + 1];
        for (int b = 1; b < 66; ++b) count[b] += count[b - 1];
        std::vector<int32_t> sorted(list.size());
        for (int32_t t : list) sorted[count[64 - coupons_of(t)]++] = t;
        list.swap(sorted);
    };
    sort_by_coupons(list_fast);
    sort_by_coupons(list_lagged);

    // Chained tables.  The kernel's wave w walks units w, w + W, w + 2W, ... (W = waves of the launch), so the rows of a pair
    // of trades (one per group of a wave) go to consecutive "rounds" of one wave column; pairs are dealt to the columns
    // longest first, always to the shortest column.
    auto deal_chains = [&](int set, int waves_per_block) {
        std::vector<int32_t>& list = L.trades[set];
        std::stable_sort(list.begin(), list.end(), [&](int32_t a, int32_t b) { return rows_of(a) > rows_of(b); });
        const int G = fast_kernel_groups();
        const int64_t W = static_cast<int64_t>(cu) * waves_per_block;
        // pass 1: the wave column and first round of every pair - always the shortest column, the lowest-numbered one among
        // equals (a heap of (height, column): with tens of thousands of pairs and thousands of columns a linear search
        // per pair was most of the upload's host time for books of long legs)
        const size_t n_pairs = (list.size() + static_cast<size_t>(G) - 1) / static_cast<size_t>(G);
        std::vector<int64_t> pair_col(n_pairs), pair_round(n_pairs);
        typedef std::pair<int64_t, int64_t> HW;                                  // (height, column)
        std::priority_queue<HW, std::vector<HW>, std::greater<HW>> heap;
        for (int64_t w = 0; w < W; ++w) heap.push(HW(0, w));
        int64_t rounds = 0;
        for (size_t pi = 0; pi < n_pairs; ++pi) {
            const HW top = heap.top();
            heap.pop();
            const int64_t len = rows_of(list[pi * static_cast<size_t>(G)]);     // the longest of the pair (sorted)
            pair_col[pi] = top.second; pair_round[pi] = top.first;
            heap.push(HW(top.first + len, top.second));
            rounds = std::max(rounds, top.first + len);
        }
        // pass 2: the rows
        const size_t total = static_cast<size_t>(rounds * W * G);
        std::vector<int32_t>&p_trade = L.chain_trade[set], &p_first = L.chain_first[set];
        std::vector<uint8_t>& p_more = L.chain_more[set];
        p_trade.assign(total, -1); p_first.assign(total, 0); p_more.assign(total, 0);
        for (size_t pi = 0; pi < n_pairs; ++pi) {
            const size_t i = pi * static_cast<size_t>(G);
            const int64_t len = rows_of(list[i]);
            for (int64_t j = 0; j < len; ++j)
                for (int g = 0; g < G; ++g) {
                    const size_t at = static_cast<size_t>(((pair_round[pi] + j) * W + pair_col[pi]) * G + g);
                    p_more[at] = j + 1 < len ? 1 : 0;
                    if (i + static_cast<size_t>(g) >= list.size()) continue;          // an odd trade out: the slot stays empty
                    const int64_t t = list[i + static_cast<size_t>(g)];
                    p_first[at] = static_cast<int32_t>(j * kRowSlots);
                    // results are written after the chain's last row, by the row's trade index: an empty padding row of
                    // the shorter trade still has to carry that index
                    if (j < rows_of(t) || j + 1 == len) p_trade[at] = static_cast<int32_t>(t);
                }
        }
        return cu;
    };
    if (!list_long.empty()) tc.chained_blocks = deal_chains(S_CHAINED, kFastThreads / 64);
    // payment-lag legs of 33-128 coupons: chains of rows for the grid of the variant
    if (!list_lagged_long.empty()) tc.lagged_chained_blocks = deal_chains(S_LAGGED_CHAINED, fast_kernel_threads(true) / 64);
    if (!list_lagged.empty() || !list_lagged_long.empty()) {
        // the variant's per-wave stash is sized for the grids these rows can be launched on: the chained rows' fixed grid, or
        // as many blocks as the one-row trades fill (557 KB per block: a batch with a handful of such trades must not pin 143 MB)
        const int waves = fast_kernel_threads(true) / 64, G = fast_kernel_groups();
        const int64_t units = (static_cast<int64_t>(list_lagged.size()) + G - 1) / G;
        const int need = static_cast<int>(std::min<int64_t>(cu, (units + waves - 1) / waves));
        tc.lag_scratch = true;
        tc.lag_blocks = std::max({1, need, tc.lagged_chained_blocks});
    }

    // lite tables (kernels.hpp, LiteRowsDev): segments of equal row count, longest coupon counts first - one for the trades of
    // the 32-slot row tables, one (with accrual ends and notional multipliers) for trades with payment lag or per-coupon
    // notionals of at most 390 coupons per leg (26 rows).  Rows per trade are rounded up to one of kLiteSegments row counts
    // (the kernel keeps one segment per distinct count).
    auto lay_lite = [&](std::vector<int32_t> (&seg_trades)[kLiteSegments], int set) {
        constexpr int S = kLiteSlots, G = 64 / kLiteSlots;
        LiteRowsDev& lt = L.lite[set];
        int64_t units = 0, rows = 0;
        int used[kLiteSegments];                      // the non-empty row counts, longest first, packed to the front
        lt.n_seg = 0;
        for (int k = 0; k < kLiteSegments; ++k) {
            lt.seg_rows[k] = 1; lt.seg_unit0[k] = 0; lt.seg_row0[k] = 0;
            if (seg_trades[k].empty()) continue;
            used[lt.n_seg++] = k;
        }
        for (int j = 0; j < lt.n_seg; ++j) {
            const int k = used[j];
            sort_by_coupons(seg_trades[k]);
            lt.seg_rows[j] = static_cast<int>(kLiteRowBuckets[kLiteSegments - 1 - k]);
            lt.seg_unit0[j] = units;
            lt.seg_row0[j] = rows;
            const int64_t seg_units = (static_cast<int64_t>(seg_trades[k].size()) + G - 1) / G;
            units += seg_units;
            rows += seg_units * G * lt.seg_rows[j];
        }
        for (int j = lt.n_seg; j < kLiteSegments; ++j) { lt.seg_unit0[j] = units; lt.seg_row0[j] = rows; }   // (never reached)
        lt.n_units = units;
        if (rows * S > static_cast<int64_t>(UINT32_MAX)) { L.too_many_rows = true; return; }   // the kernel indexes with 32 bits
        const size_t n_slots = static_cast<size_t>(units) * G, n_rows = static_cast<size_t>(rows);
        std::vector<int32_t>& slot_trade = L.trades[set];
        std::vector<int32_t>& row_slot = L.lite_row_slot[set];
        std::vector<uint8_t>& row_piece = L.lite_row_piece[set];
        slot_trade.assign(n_slots, -1); row_slot.assign(n_rows, -1); row_piece.assign(n_rows, 0);
        for (int j = 0; j < lt.n_seg; ++j) {
            const int k = used[j];
            const int R = lt.seg_rows[j];
            const size_t slot0 = static_cast<size_t>(lt.seg_unit0[j]) * G, row0 = static_cast<size_t>(lt.seg_row0[j]);
            for (size_t i = 0; i < seg_trades[k].size(); ++i) slot_trade[slot0 + i] = seg_trades[k][i];
            const size_t slots_here = ((seg_trades[k].size() + G - 1) / G) * G;
            for (size_t i = 0; i < slots_here; ++i)
                for (int r = 0; r < R; ++r) {
                    row_slot[row0 + i * static_cast<size_t>(R) + static_cast<size_t>(r)] = static_cast<int32_t>(slot0 + i);
                    row_piece[row0 + i * static_cast<size_t>(R) + static_cast<size_t>(r)] = static_cast<uint8_t>(r);
                }
        }
    };
    lay_lite(seg_plain, S_LITE);
    if (!L.too_many_rows && nonlite.size() > nonlite_b.size()) lay_lite(seg_lag, S_LITE_LAG);

    tc.rows = static_cast<int64_t>(list_fast.size());
    tc.chained_rows = static_cast<int64_t>(L.chain_trade[S_CHAINED].size());
    tc.lagged_rows = static_cast<int64_t>(list_lagged.size());
    tc.lagged_chained_rows = static_cast<int64_t>(L.chain_trade[S_LAGGED_CHAINED].size());
    tc.lite_units = L.lite[S_LITE].n_units; tc.lite_lag_units = L.lite[S_LITE_LAG].n_units;
    tc.n_general = static_cast<int64_t>(list_general.size()); tc.n_general_b = static_cast<int64_t>(general_b.size());
    tc.n_rest = static_cast<int64_t>(list_rest.size());
    tc.n_nonlite = static_cast<int64_t>(nonlite.size()); tc.n_nonlite_b = static_cast<int64_t>(nonlite_b.size());
    return L;
}

}  // namespace route
}  // namespace adr
