// Stand-alone sanitizer driver for adr_yoy_subbook_ladders_host (CPU only; not a test of the suite and not for a GPU
// machine): calls the host twin on exactly sized heap buffers over desks of 1, 63, 64, 0, 65, 129, 0 swaps - legs of 0 to
// 70 coupons and 0 to 70 fixed flows, dead flows, coupons before the first and beyond the last inflation pillar -, the three
// discount schemes times the two inflation schemes, P_i = 1, 12 and 64, with and without GAMMA, and over the refusals.  Build
// the library's sources and this file with -fsanitize=address,undefined on the host side and run it:
//   make -C adrates_amd/csrc OBJDIR=build_asan OUT=build_asan/libadrates_asan.so EXTRA="-Xarch_host -fsanitize=address,undefined"
//   clang++ -std=c++17 -g -fsanitize=address,undefined -Iinclude tools/asan_yoy_sub_book_ladders.cpp \
//           -Ladrates_amd/csrc/build_asan -ladrates_asan -Wl,-rpath,$PWD/adrates_amd/csrc/build_asan -o build_asan/driver
//   ASAN_OPTIONS=detect_leaks=0 build_asan/driver      (the HIP runtime the library links keeps its start-up allocations)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "adrates.h"

namespace {

struct Book {
    std::vector<int64_t> fix_off{0}, cpn_off{0};
    std::vector<double> fix_tp, fix_pay, tp, ts, te, scale, spread;
    int64_t n() const { return static_cast<int64_t>(fix_off.size()) - 1; }
    // the field-major coupon array [ADR_YOY_FIELDS][m]
    std::vector<double> cpn() const {
        std::vector<double> c;
        for (const auto* f : {&tp, &ts, &te, &scale, &spread}) c.insert(c.end(), f->begin(), f->end());
        return c;
    }
};

// Swap i: monthly coupons on the year-on-year ratio from a start that runs from seasoned to beyond the last pillar, and on
// every second swap fixed flows; every fifth swap has neither.
void add_swap(Book& b, int i) {
    const int coupons = i % 5 == 4 ? 0 : (i % 13 == 0 ? 70 : 1 + i % 9), flows = i % 2 == 0 || i % 5 == 4 ? 0 : (i % 17 == 1 ? 70 : 1 + i % 4);
    const double start = -1.6 + 0.7 * (i % 60), sign = i % 3 ? 1.0 : -1.0;
    for (int c = 1; c <= coupons; ++c) {
        const double e = start + c / 12.0;
        b.tp.push_back(e + (i % 2) * 2.0 / 365.0);
        b.ts.push_back(e - 1.0);
        b.te.push_back(e);
        b.scale.push_back(sign * 1e5 * (1 + i % 7) / 12.0);
        b.spread.push_back(0.001 * (i % 3));
    }
    for (int f = 0; f < flows; ++f) {
        b.fix_tp.push_back(-0.25 + 0.5 * f + 0.01 * (i % 10));
        b.fix_pay.push_back(-sign * 1e3 * (1 + f % 3));
    }
    b.cpn_off.push_back(static_cast<int64_t>(b.tp.size()));
    b.fix_off.push_back(static_cast<int64_t>(b.fix_tp.size()));
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        ++failures;
        std::printf("FAILED: %s (%s)\n", what, adr_last_error());
    }
}

}  // namespace

int main() {
    const int K = 41, P = 6;
    std::vector<double> times(K), dfs(K), jac(static_cast<size_t>(K) * P), hess(static_cast<size_t>(K) * P * P);
    for (int k = 0; k < K; ++k) {
        times[k] = 0.75 * k;
        dfs[k] = std::exp(-0.04 * times[k]);
        for (int p = 0; p < P; ++p) {
            jac[static_cast<size_t>(k) * P + p] = k == 0 ? 0.0 : -times[k] * dfs[k] * (p <= k % P ? 0.3 : 0.05);
            for (int q = 0; q < P; ++q)
                hess[(static_cast<size_t>(k) * P + p) * P + q] = k == 0 ? 0.0 : times[k] * times[k] * dfs[k] * 0.01 / (1 + std::abs(p - q));
        }
    }
    const int sizes[] = {1, 63, 64, 0, 65, 129, 0};
    const int B = 7;
    Book b;
    std::vector<int64_t> sub_off{0};
    int i = 0;
    for (int d = 0; d < B; ++d) {
        for (int j = 0; j < sizes[d]; ++j, ++i) add_swap(b, i);
        sub_off.push_back(b.n());
    }
    const std::vector<double> cpn = b.cpn();
    const int64_t n_fix = static_cast<int64_t>(b.fix_tp.size()), m = static_cast<int64_t>(b.tp.size());
    const int disc[] = {ADR_INTERP_FLAT_FWD_RATES, ADR_INTERP_LINEAR_FWD_RATES, ADR_INTERP_LINEAR_ZERO_RATES};
    const int infl[] = {ADR_INTERP_FLAT_FWD_RATES, ADR_INTERP_LINEAR_ZERO_RATES};
    std::vector<double> T, rate, out;
    auto call = [&](int dm, int im, const Book& x, const std::vector<double>& c, const std::vector<int64_t>& off, uint32_t mask) {
        return adr_yoy_subbook_ladders_host(dm, K, P, times.data(), dfs.data(), jac.data(), (mask & ADR_REQ_GAMMA) ? hess.data() : nullptr,
                                            im, static_cast<int>(T.size()), T.data(), rate.data(), x.n(), n_fix, x.fix_off.data(),
                                            x.fix_tp.data(), x.fix_pay.data(), m, x.cpn_off.data(), c.data(), B, off.data(), mask,
                                            out.data());
    };
    for (int Pi : {1, 12, 64}) {
        T.assign(Pi, 0.0);
        rate.assign(Pi, 0.0);
        for (int k = 0; k < Pi; ++k) {
            T[k] = Pi == 1 ? 3.0 : 0.5 + 39.5 * k / (Pi - 1);
            rate[k] = 0.03 + 0.006 * std::sin(0.2 * T[k]);
        }
        const int Q = P + Pi;
        const size_t stride = 1 + Q + static_cast<size_t>(Q) * Q;
        out.assign(B * stride, 0.0);
        for (int dm : disc)
            for (int im : infl)
                for (uint32_t mask : {uint32_t(ADR_REQ_VALUE), uint32_t(ADR_REQ_VALUE | ADR_REQ_DELTA), uint32_t(ADR_REQ_VALUE | ADR_REQ_DELTA | ADR_REQ_GAMMA)}) {
                    expect(call(dm, im, b, cpn, sub_off, mask) == ADR_OK, "a valid call");
                    bool finite = true;
                    for (double v : out) finite = finite && std::isfinite(v);
                    expect(finite, "finite rows");
                    expect(out[3 * stride] == 0.0 && out[stride] != 0.0, "an empty desk is zero, desk 1 is not");
                }
    }
    // the refusals (P_i = 64 still set), each on a copy with one thing wrong
    const int LZ = ADR_INTERP_LINEAR_ZERO_RATES;
    expect(call(LZ, ADR_INTERP_LINEAR_FWD_RATES, b, cpn, sub_off, 7) == ADR_ERR_UNSUPPORTED, "an inflation scheme that is not implemented");
    expect(call(3, LZ, b, cpn, sub_off, 7) == ADR_ERR_UNSUPPORTED, "a discount scheme that is not implemented");
    std::vector<double> c = cpn;
    c[3] = NAN;
    expect(call(LZ, LZ, b, c, sub_off, 7) == ADR_ERR_INVALID, "a non-finite coupon field");
    Book x = b;
    x.fix_pay[2] = INFINITY;
    expect(call(LZ, LZ, x, cpn, sub_off, 7) == ADR_ERR_INVALID, "a non-finite fixed amount");
    x = b;
    x.cpn_off[5] = x.cpn_off[6] + 1;
    expect(call(LZ, LZ, x, cpn, sub_off, 7) == ADR_ERR_INVALID, "decreasing coupon offsets");
    x = b;
    x.fix_off.back() += 1;
    expect(call(LZ, LZ, x, cpn, sub_off, 7) == ADR_ERR_INVALID, "fixed offsets that do not end at the flow count");
    std::vector<int64_t> bad = sub_off;
    bad[2] = bad[1] - 1;
    expect(call(LZ, LZ, b, cpn, bad, 7) == ADR_ERR_INVALID && std::strstr(adr_last_error(), "sub-book"), "decreasing sub_off");
    const double t1 = T[1];
    T[1] = T[0];
    expect(call(LZ, LZ, b, cpn, sub_off, 7) == ADR_ERR_INVALID, "pillar times that do not increase");
    T[1] = t1;
    rate[7] = -1.0;
    expect(call(LZ, LZ, b, cpn, sub_off, 7) == ADR_ERR_INVALID, "a breakeven rate of -1");
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
