// Stand-alone sanitizer driver for the schedule-group search (adrates_amd/csrc/schedule_groups.cpp; CPU only, not a test of
// the suite and not for a GPU machine): a few thousand generated swaps on exactly sized heap buffers - shared schedules of 1
// to 32 coupons, members with proportional payments, zero-coupon members, outliers, empty legs and a list that leaves
// trades out - through build_schedule_groups, with the groups checked against the generator; then every book's groups
// through build_group_tables (the host image of the grouped route's device tables) at minimum group sizes 2 and 64, segment
// lengths 1, 16 and 33 and a threshold that rejects the batch, with the tables' invariants checked.  Both are host C++
// with no HIP, so the two files build on their own:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iadrates_amd/csrc \
//           tools/asan_schedule_groups.cpp adrates_amd/csrc/schedule_groups.cpp -o build_asan/schedule_groups_driver
//   build_asan/schedule_groups_driver
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "schedule_groups.hpp"

namespace {

struct Book {
    std::vector<int64_t> fix_off{0}, flt_off{0};
    std::vector<double> fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, notional, spread, fix_sign, flt_sign;
    std::vector<int> schedule;          // the generator's schedule and shape of the trade, -1: must stay ungrouped
    std::vector<char> any_shape;        // a fixed leg of zeros joins whichever group its schedule has
};

// Trade i on schedule s: m = 1 + s % 32 coupons per leg (schedule 7: no fixed leg, 11: no float leg).
void add_trade(Book& b, int i, int s) {
    const int m = 1 + s % 32;
    const double years = 0.3 * m + 0.01 * s, N = 1e6 * (1 + i % 41), c = 0.01 + 0.001 * (i % 57);
    const bool zero = i % 97 == 5, outlier = i % 89 == 3, zero_last = i % 101 == 7;
    if (s != 11)
        for (int j = 0; j < m; ++j) {
            b.flt_ts.push_back(years * j / m);
            b.flt_te.push_back(years * (j + 1) / m);
            b.flt_tp.push_back(years * (j + 1) / m);
            b.flt_alpha.push_back(years / m);
        }
    if (s != 7)
        for (int j = 0; j < m; ++j) {
            double pay = zero ? 0.0 : N * c * (years / m) * (1.0 + 0.01 * std::sin(1.0 + j));
            if (outlier && j == m / 2) pay *= 1.01;
            if (zero_last && j == m - 1) pay = 0.0;
            b.fix_tp.push_back(years * (j + 1) / m);
            b.fix_pay.push_back(pay);
        }
    const bool has_fix = s != 7;
    // one coupon: any payment has the shape.  A last payment of zero after others never joins; trades with the same payment
    // 1 % up are proportional to each other: they may form the group (when the first of them is the schedule's lowest trade,
    // the shape is theirs and the others stay out) but never share one with the others.
    const bool alone = has_fix && !zero && m > 1 && zero_last;
    const bool apart = has_fix && !zero && m > 1 && outlier;
    b.fix_off.push_back(static_cast<int64_t>(b.fix_tp.size()));
    b.flt_off.push_back(static_cast<int64_t>(b.flt_tp.size()));
    b.notional.push_back(N);
    b.spread.push_back(s % 3 == 0 ? 0.001 : 0.0);
    b.fix_sign.push_back(i % 2 ? 1.0 : -1.0);
    b.flt_sign.push_back(i % 2 ? -1.0 : 1.0);
    b.any_shape.push_back(has_fix && zero);
    b.schedule.push_back(alone ? -1 : (apart ? 100000 + s : s));
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

// exactly sized heap copies: an access one element past any array is the sanitizer's to report
template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

bool all_empty(const adr::GroupTables& T) {
    return T.used_groups == 0 && T.used_trades == 0 && T.rec.empty() && T.seg.empty() && T.sum_f.empty() && T.sum_x.empty() &&
           T.rest.empty() && T.fix_off.empty() && T.flt_off.empty() && T.fix_tp.empty() && T.fix_pay.empty() && T.flt_tp.empty() &&
           T.flt_ts.empty() && T.flt_te.empty() && T.flt_alpha.empty() && T.notional.empty() && T.spread.empty() && T.sign.empty() &&
           T.rows.empty();
}

// The tables of the groups of at least `min_group` trades, `segment` records per segment, for the row order rows[0 .. n_rows).
void check_tables(const adr::ScheduleGroups& G, const int32_t* rows, int64_t n_rows, int min_group, int segment) {
    int64_t want_groups = 0, want_trades = 0;
    for (int32_t s : G.size)
        if (s >= min_group) { ++want_groups; want_trades += s; }
    // a threshold the batch misses: route not taken
    expect(all_empty(adr::build_group_tables(G, rows, n_rows, min_group, want_trades + 1, segment)), "a rejected batch has no tables");
    const adr::GroupTables T = adr::build_group_tables(G, rows, n_rows, min_group, want_trades, segment);
    expect(T.used_groups == want_groups, "groups in use");
    if (want_groups == 0) { expect(all_empty(T), "no group in use: no tables"); return; }
    expect(T.used_trades == want_trades && T.rec.size() == static_cast<size_t>(want_trades), "one record per grouped trade");
    const size_t ng = static_cast<size_t>(want_groups), nr = T.rec.size();
    const auto rec = exact(T.rec);
    const auto seg = exact(T.seg);
    const auto sum_f = exact(T.sum_f), sum_x = exact(T.sum_x);
    expect(T.sum_f.size() == ng && T.sum_x.size() == ng, "one pair of sums per group");

    // records: sorted by group, then by trade; a new group is one old group; the coefficients are the search's
    bool sorted = true, coeff = true, one_old = true;
    std::vector<int32_t> old_of(ng, -1);
    std::vector<char> grouped(G.group_of.size(), 0);
    for (size_t i = 0; i < nr; ++i) {
        const adr::GroupRecord& r = rec[i];
        if (r.group < 0 || static_cast<size_t>(r.group) >= ng || r.trade < 0 || static_cast<size_t>(r.trade) >= G.group_of.size()) { sorted = false; break; }
        if (i > 0) sorted &= rec[i - 1].group < r.group || (rec[i - 1].group == r.group && rec[i - 1].trade < r.trade);
        coeff &= same_bits(r.cF, G.cF[static_cast<size_t>(r.trade)]) && same_bits(r.cX, G.cX[static_cast<size_t>(r.trade)]);
        int32_t& old = old_of[static_cast<size_t>(r.group)];
        if (old < 0) old = G.group_of[static_cast<size_t>(r.trade)];
        one_old &= old >= 0 && old == G.group_of[static_cast<size_t>(r.trade)] && G.size[static_cast<size_t>(old)] >= min_group;
        grouped[static_cast<size_t>(r.trade)] = 1;
    }
    expect(sorted, "records sorted by group, then by trade");
    if (!sorted) return;
    expect(coeff, "records carry the members' coefficients");
    expect(one_old, "a group in use is one group of the search, of at least the minimum size");

    // segments: inside one group, no longer than asked, tiling the records once
    bool inside = true, tiled = true;
    int64_t cursor = 0;
    for (size_t k = 0; k < T.seg.size(); ++k) {
        const adr::GroupSegment& sg = seg[k];
        tiled &= sg.first == cursor && sg.count >= 1 && sg.count <= segment && sg.first + static_cast<int64_t>(sg.count) <= static_cast<int64_t>(nr);
        if (!tiled) break;
        for (int32_t i = sg.first; i < sg.first + sg.count; ++i) inside &= rec[static_cast<size_t>(i)].group == sg.group;
        cursor += sg.count;
    }
    expect(tiled && cursor == static_cast<int64_t>(nr), "segments tile the records once, none longer than asked");
    expect(inside, "a segment lies inside one group");

    // grouped trades and outside rows partition the row order; the outside rows keep its order
    bool partition = true;
    size_t at = 0;
    int64_t grouped_rows = 0;
    for (int64_t i = 0; i < n_rows; ++i) {
        const int32_t t = rows[i];
        const bool out = at < T.rest.size() && T.rest[at] == t;
        if (out) ++at;
        if (grouped[static_cast<size_t>(t)]) ++grouped_rows;
        partition &= out != (grouped[static_cast<size_t>(t)] != 0);
    }
    expect(partition && at == T.rest.size() && grouped_rows == want_trades, "grouped trades and outside rows partition the row order");

    // sums: bit-equal to the in-order sum of the group's records
    bool sums = true;
    {
        std::vector<double> f(ng, 0.0), x(ng, 0.0);
        for (size_t i = 0; i < nr; ++i) { f[static_cast<size_t>(rec[i].group)] += rec[i].cF; x[static_cast<size_t>(rec[i].group)] += rec[i].cX; }
        for (size_t g = 0; g < ng; ++g) sums &= same_bits(f[g], sum_f[g]) && same_bits(x[g], sum_x[g]);
    }
    expect(sums, "sums are the in-order sums of the records");

    // basis batch: two pseudo-trades per group in use, offsets ending at the flow counts
    const size_t nfix = T.fix_tp.size(), nflt = T.flt_tp.size();
    expect(T.fix_off.size() == 2 * ng + 1 && T.flt_off.size() == 2 * ng + 1 && T.fix_off[0] == 0 && T.flt_off[0] == 0, "basis offsets");
    expect(T.fix_off.back() == static_cast<int64_t>(nfix) && T.fix_pay.size() == nfix, "basis fixed offsets end at the flow count");
    expect(T.flt_off.back() == static_cast<int64_t>(nflt) && T.flt_ts.size() == nflt && T.flt_te.size() == nflt && T.flt_alpha.size() == nflt,
           "basis float offsets end at the flow count");
    bool rising = true, identity = T.rows.size() == 2 * ng, leg_of_group = true;
    for (size_t k = 0; k < 2 * ng && T.fix_off.size() == 2 * ng + 1; ++k) rising &= T.fix_off[k] <= T.fix_off[k + 1] && T.flt_off[k] <= T.flt_off[k + 1];
    for (size_t k = 0; k < T.rows.size(); ++k) identity &= T.rows[k] == static_cast<int32_t>(k);
    for (size_t g = 0; g < ng && rising && T.fix_off.size() == 2 * ng + 1; ++g) {      // the legs are those of the search's group
        const size_t o = static_cast<size_t>(old_of[g]);
        leg_of_group &= T.flt_off[2 * g + 1] - T.flt_off[2 * g] == G.flt_off[2 * o + 1] - G.flt_off[2 * o] &&
                        T.fix_off[2 * g + 2] - T.fix_off[2 * g + 1] == G.fix_off[2 * o + 2] - G.fix_off[2 * o + 1] &&
                        same_bits(T.spread[2 * g], G.spread[2 * o]);
    }
    expect(rising && identity && leg_of_group, "basis batch: the legs of the groups in use, identity row list");
    expect(T.notional.size() == 2 * ng && T.spread.size() == 2 * ng && T.sign.size() == 2 * ng, "basis per-trade arrays");
}

void run(int n, int n_schedules, int skip_every) {
    Book b;
    for (int i = 0; i < n; ++i) add_trade(b, i, (i * 7 + i / 13) % n_schedules);
    std::vector<int32_t> eligible;
    for (int i = 0; i < n; ++i)
        if (skip_every == 0 || i % skip_every != 0) eligible.push_back(i);
    auto fo = exact(b.fix_off), lo = exact(b.flt_off);
    auto ftp = exact(b.fix_tp), fpay = exact(b.fix_pay), ltp = exact(b.flt_tp), lts = exact(b.flt_ts), lte = exact(b.flt_te), la = exact(b.flt_alpha);
    auto nn = exact(b.notional), sp = exact(b.spread), fs = exact(b.fix_sign), ls = exact(b.flt_sign);
    auto el = exact(eligible);
    const adr::CsrHost csr{n, fo.get(), lo.get(), ftp.get(), fpay.get(), ltp.get(), lts.get(), lte.get(), la.get(), nn.get(), sp.get(), fs.get(), ls.get()};
    adr::ScheduleGroups G;
    adr::build_schedule_groups(csr, el.get(), static_cast<int64_t>(eligible.size()), G);

    std::vector<int> schedule_of_group(static_cast<size_t>(G.n_groups), -2);
    int64_t grouped = 0;
    bool consistent = true, outside = true;
    for (int i = 0; i < n; ++i) {
        const int32_t g = G.group_of[static_cast<size_t>(i)];
        const bool listed = skip_every == 0 || i % skip_every != 0;
        if (g < 0) continue;
        ++grouped;
        outside &= listed && b.schedule[static_cast<size_t>(i)] >= 0;
        if (b.any_shape[static_cast<size_t>(i)]) continue;
        int& s = schedule_of_group[static_cast<size_t>(g)];
        if (s == -2) s = b.schedule[static_cast<size_t>(i)];
        consistent &= s == b.schedule[static_cast<size_t>(i)];
    }
    expect(consistent, "a group holds trades of one schedule and shape");
    expect(outside, "no zero-last or unlisted trade is grouped");
    expect(grouped == G.n_grouped, "n_grouped counts the grouped trades");
    expect(G.fix_off.size() == static_cast<size_t>(2 * G.n_groups + 1) && G.flt_off.size() == G.fix_off.size(), "basis offsets");
    expect(G.fix_off.back() == static_cast<int64_t>(G.fix_tp.size()) && G.flt_off.back() == static_cast<int64_t>(G.flt_tp.size()), "basis flows");
    int64_t sizes = 0;
    for (int32_t s : G.size) { sizes += s; expect(s >= 2, "group of at least two"); }
    expect(sizes == G.n_grouped, "sizes add up");
    // the tables of the grouped route, for a row order that is not the trade order (the listed trades, last first)
    const std::vector<int32_t> order(eligible.rbegin(), eligible.rend());
    const auto rows = exact(order);
    for (int min_group : {2, 64})
        for (int segment : {1, 16, 33}) check_tables(G, rows.get(), static_cast<int64_t>(order.size()), min_group, segment);
    std::printf("n = %d, %d schedules, skip %d: %lld groups, %lld grouped\n", n, n_schedules, skip_every,
                static_cast<long long>(G.n_groups), static_cast<long long>(G.n_grouped));
}

}  // namespace

int main() {
    run(0, 1, 0);
    run(1, 1, 0);
    run(2, 1, 0);
    run(5000, 97, 0);
    run(5000, 2500, 0);          // most schedules hold one or two trades
    run(20000, 40, 3);           // several hash partitions, a third of the trades not listed
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("schedule groups: all checks passed\n");
    return 0;
}
