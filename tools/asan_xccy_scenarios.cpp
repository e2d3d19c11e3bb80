// Stand-alone sanitizer driver for adr_xccy_scenario_pv_host and adr_xccy_scenario_subbook_pv_host (CPU only; not a test of the
// suite and not for a GPU machine): calls the host twins on exactly sized heap buffers over desks of 1, 63, 64, 0, 65, 129, 0
// trades - legs of 0 to 70 coupons and 0 to 3 fixed flows, dead flows, dates before the first and beyond the last knot -, the
// five scheme pairs, table sizes (2, 2), (40, 5) and (5, 300), every broadcast combination, with and without per-trade rows and
// weights, and over the refusals.  Build the library's sources and this file with -fsanitize=address,undefined on the host side
// and run it:
//   make -C adrates_amd/csrc OBJDIR=build_asan OUT=build_asan/libadrates_asan.so EXTRA="-Xarch_host -fsanitize=address,undefined"
//   clang++ -std=c++17 -g -fsanitize=address,undefined -Iinclude tools/asan_xccy_scenarios.cpp \
//           -Ladrates_amd/csrc/build_asan -ladrates_asan -Wl,-rpath,$PWD/adrates_amd/csrc/build_asan -o build_asan/driver
//   ASAN_OPTIONS=detect_leaks=0 build_asan/driver      (the HIP runtime the library links keeps its start-up allocations)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "adrates.h"

namespace {

struct Book {
    std::vector<int64_t> fix_off{0}, flt_off{0};
    std::vector<double> fix_tp, fix_pay, tp, ts, te, alpha, weight, notional, spread, fix_sign, flt_sign;
    int64_t n() const { return static_cast<int64_t>(notional.size()); }
};

// Trade i: quarterly coupons from a start that runs from seasoned to beyond the last knot, a payment lag on every third trade,
// a coupon that does not accrue on every fourth, up to three fixed flows; every fifth trade has neither leg.
void add_trade(Book& b, int i) {
    const int coupons = i % 5 == 4 ? 0 : (i % 13 == 0 ? 70 : 1 + i % 9), flows = i % 5 == 4 ? 0 : i % 4;
    const double start = -1.6 + 0.7 * (i % 60);
    for (int c = 1; c <= coupons; ++c) {
        const double e = start + 0.25 * c;
        b.ts.push_back(e - 0.25);
        b.te.push_back(e);
        b.tp.push_back(e + (i % 3 == 0 ? 2.0 / 365.0 : 0.0));
        b.alpha.push_back(i % 4 == 3 && c == 2 ? 0.0 : 0.25);
        b.weight.push_back(1.0 + 0.01 * (c % 7));
    }
    for (int f = 0; f < flows; ++f) {
        b.fix_tp.push_back(start + 0.25 * (f + 1) + (f == 2 ? 0.01 : 0.0));
        b.fix_pay.push_back(1000.0 * (f + 1));
    }
    b.flt_off.push_back(static_cast<int64_t>(b.tp.size()));
    b.fix_off.push_back(static_cast<int64_t>(b.fix_tp.size()));
    b.notional.push_back(std::pow(10.0, i % 9));
    b.spread.push_back(1e-3 * (i % 7 - 3));
    b.fix_sign.push_back(i % 2 ? 1.0 : -1.0);
    b.flt_sign.push_back(i % 3 ? 1.0 : -1.0);
}

struct Table {
    std::vector<double> times, dfs;
    int K, rows;
};

Table table(int K, int rows, double step, double rate) {
    Table t{std::vector<double>(K), std::vector<double>(static_cast<size_t>(rows) * K), K, rows};
    for (int k = 0; k < K; ++k) t.times[k] = step * k;
    for (int s = 0; s < rows; ++s)
        for (int k = 0; k < K; ++k) t.dfs[static_cast<size_t>(s) * K + k] = std::exp(-(rate + 0.002 * s) * t.times[k]);
    return t;
}

int failures = 0;

void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        std::printf("FAILED: %s (%s)\n", what, adr_last_error());
    }
}

int run(const Book& b, int fm, const Table& f, int xm, const Table& x, int S, bool per_trade, bool weighted,
        const std::vector<int64_t>* sub_off, std::vector<double>* book_out = nullptr) {
    const int64_t n = b.n();
    const size_t B = sub_off ? sub_off->size() - 1 : 1;
    std::vector<double> pv(per_trade ? static_cast<size_t>(n) * S : 0), book(B * S);
    const double* w = weighted ? b.weight.data() : nullptr;
    int rc;
    if (sub_off)
        rc = adr_xccy_scenario_subbook_pv_host(fm, f.K, f.times.data(), f.rows, f.dfs.data(), xm, x.K, x.times.data(), x.rows, x.dfs.data(), S, n,
                                               b.fix_off.data(), b.flt_off.data(), b.fix_tp.data(), b.fix_pay.data(), b.tp.data(), b.ts.data(),
                                               b.te.data(), b.alpha.data(), w, b.notional.data(), b.spread.data(), b.fix_sign.data(),
                                               b.flt_sign.data(), static_cast<int64_t>(B), sub_off->data(), per_trade ? pv.data() : nullptr,
                                               book.data(), 3);
    else
        rc = adr_xccy_scenario_pv_host(fm, f.K, f.times.data(), f.rows, f.dfs.data(), xm, x.K, x.times.data(), x.rows, x.dfs.data(), S, n,
                                       b.fix_off.data(), b.flt_off.data(), b.fix_tp.data(), b.fix_pay.data(), b.tp.data(), b.ts.data(), b.te.data(),
                                       b.alpha.data(), w, b.notional.data(), b.spread.data(), b.fix_sign.data(), b.flt_sign.data(),
                                       per_trade ? pv.data() : nullptr, book.data(), 3);
    if (rc == ADR_OK)
        for (double v : book) expect(std::isfinite(v), "a finite result");
    if (book_out) *book_out = book;
    return rc;
}

}  // namespace

int main() {
    Book b;
    const int desks[] = {1, 63, 64, 0, 65, 129, 0};
    std::vector<int64_t> sub_off{0};
    int i = 0;
    for (int d : desks) {
        for (int j = 0; j < d; ++j) add_trade(b, i++);
        sub_off.push_back(b.n());
    }
    const int pairs[5][2] = {{1, 1}, {1, 4}, {4, 1}, {4, 4}, {2, 2}};
    const int shapes[3][2] = {{2, 2}, {40, 5}, {5, 300}};
    int calls = 0;
    for (const auto& p : pairs)
        for (const auto& k : shapes)
            for (int bc = 0; bc < 4; ++bc) {
                const int S = bc == 3 ? 1 : 5;
                const Table f = table(k[0], bc & 1 ? 1 : S, k[0] == 2 ? 30.0 : 0.5, 0.03), x = table(k[1], bc & 2 ? 1 : S, k[1] == 2 ? 30.0 : 0.125, 0.02);
                for (int form = 0; form < 4; ++form) {
                    std::vector<double> whole, rows;
                    expect(run(b, p[0], f, p[1], x, S, form & 1, form & 2, nullptr, &whole) == ADR_OK, "adr_xccy_scenario_pv_host");
                    expect(run(b, p[0], f, p[1], x, S, form & 1, form & 2, &sub_off, &rows) == ADR_OK, "adr_xccy_scenario_subbook_pv_host");
                    for (int s = 0; s < S; ++s) expect(rows[3 * S + s] == 0.0 && !std::signbit(rows[3 * S + s]), "an empty desk is +0.0");
                    calls += 2;
                }
            }
    // the refusals read nothing they should not
    const Table f = table(40, 3, 0.5, 0.03), x = table(5, 3, 2.0, 0.02);
    expect(run(b, 2, f, 1, x, 3, true, true, nullptr) == ADR_ERR_UNSUPPORTED, "LINEAR_FWD_RATES beside a log scheme");
    expect(run(b, 1, f, 3, x, 3, true, true, nullptr) == ADR_ERR_INVALID, "an unknown scheme");
    expect(run(b, 1, f, 1, x, 4, true, true, nullptr) == ADR_ERR_INVALID, "S_f that is neither 1 nor S");
    std::vector<int64_t> bad = sub_off;
    bad[2] = bad[3] + 1;
    expect(run(b, 1, f, 1, x, 3, true, true, &bad) == ADR_ERR_INVALID, "decreasing sub-book offsets");
    Table neg = x;
    neg.dfs[7] = -1.0;
    expect(run(b, 1, f, 1, neg, 3, false, false, nullptr) == ADR_ERR_INVALID, "a discount factor that is not positive");
    Book broken = b;
    broken.flt_off[5] = broken.flt_off[6] + 1;
    expect(run(broken, 1, f, 1, x, 3, false, false, nullptr) == ADR_ERR_INVALID, "decreasing leg offsets");
    std::printf("%d calls on %lld trades, %d failures\n", calls, static_cast<long long>(b.n()), failures);
    return failures ? 1 : 0;
}
