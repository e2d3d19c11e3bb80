// Stand-alone sanitizer driver for the schedule-group search (adrates_amd/csrc/schedule_groups.cpp; CPU only, not a test of
// the suite and not for a GPU machine): a few thousand generated swaps on exactly sized heap buffers - shared schedules of 1
// to 32 coupons, members with proportional payments, zero-coupon members, outliers, empty legs and a list that leaves
// trades out - through build_schedule_groups, with the groups checked against the generator.  The search is host C++ with
// no HIP, so the two files build on their own:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Iadrates_amd/csrc \
//           tools/asan_schedule_groups.cpp adrates_amd/csrc/schedule_groups.cpp -o build_asan/schedule_groups_driver
//   build_asan/schedule_groups_driver
#include <cmath>
#include <cstdint>
#include <cstdio>
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
