// Stand-alone sanitizer driver for adr_credit_subbook_ladders_host (CPU only; not a test of the suite and not for a GPU
// machine): calls the host twin on exactly sized heap buffers over desks of 1, 63, 64, 0, 65, 129, 0 trades - bonds and
// lag-free floaters mixed, G = 0, 1 and 32, the three schemes, with and without GAMMA - and over the refusals.  Build the
// library's sources and this file with -fsanitize=address,undefined on the host side and run it:
//   make -C adrates_amd/csrc OBJDIR=build_asan OUT=build_asan/libadrates_asan.so EXTRA="-Xarch_host -fsanitize=address,undefined"
//   clang++ -std=c++17 -g -fsanitize=address,undefined -Iinclude tools/asan_credit_sub_book_ladders.cpp \
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
    std::vector<int64_t> fix_off{0}, flt_off{0};
    std::vector<double> fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, notional, spread, fix_sign, flt_sign, z, fix_tau, flt_tau;
    std::vector<int32_t> bucket;
    int64_t n() const { return static_cast<int64_t>(notional.size()); }
};

// Trade i: a bond (annual coupons, redemption) when i is even, else a lag-free floater with its redemption as a fixed flow.
void add_trade(Book& b, int i, int bucket, double z) {
    const int years = 1 + i % 29;
    const double face = 100.0 * (1 + i % 7), off = 0.01 * (i % 50);
    if (i % 2 == 0) {
        for (int y = 1; y <= years; ++y) {
            b.fix_tp.push_back(y - off);
            b.fix_pay.push_back(face * (0.03 + 0.001 * (i % 10)) + (y == years ? face : 0.0));
            b.fix_tau.push_back((y - off) * 365.0 / 365.25);
        }
    } else {
        for (int y = 1; y <= years; ++y) {
            b.flt_ts.push_back(y - 1 + (y == 1 ? 0.0 : -off));
            b.flt_te.push_back(y - off);
            b.flt_tp.push_back(y - off);
            b.flt_alpha.push_back(y == 1 ? 1.0 - off : 1.0);
            b.flt_tau.push_back(y - off);
        }
        b.fix_tp.push_back(years - off);
        b.fix_pay.push_back(face);
        b.fix_tau.push_back(years - off);
    }
    b.fix_off.push_back(static_cast<int64_t>(b.fix_tp.size()));
    b.flt_off.push_back(static_cast<int64_t>(b.flt_tp.size()));
    b.notional.push_back(i % 2 ? face : 1.0);
    b.spread.push_back(0.002 * (i % 5));
    b.fix_sign.push_back(1.0);
    b.flt_sign.push_back(i % 11 == 0 ? -1.0 : 1.0);
    b.z.push_back(z);
    b.bucket.push_back(bucket);
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
    const int methods[] = {ADR_INTERP_FLAT_FWD_RATES, ADR_INTERP_LINEAR_FWD_RATES, ADR_INTERP_LINEAR_ZERO_RATES};
    for (int G : {0, 1, 32}) {
        Book b;
        std::vector<int64_t> sub_off{0};
        int i = 0;
        for (int d = 0; d < B; ++d) {
            // buckets ascending inside the desk: desk 4 one cell, desk 5 every cell, desk 2 unbucketed
            for (int j = 0; j < sizes[d]; ++j, ++i) {
                int g = -1;
                if (G > 0 && d == 4) g = G / 2;
                else if (G > 0 && d == 5) g = j * (G + 1) / sizes[d] - 1;
                else if (G > 0 && d != 2) g = j < sizes[d] / 3 ? 0 : G - 1;
                add_trade(b, i, g, i % 6 == 0 ? 0.0 : -0.005 + 0.085 * ((i * 37) % 100) / 100.0);
            }
            sub_off.push_back(b.n());
        }
        const int Q = P + G;
        std::vector<double> out(static_cast<size_t>(B) * (1 + Q + Q * Q));
        for (int method : methods)
            for (uint32_t mask : {uint32_t(ADR_REQ_VALUE), uint32_t(ADR_REQ_VALUE | ADR_REQ_DELTA), uint32_t(ADR_REQ_VALUE | ADR_REQ_DELTA | ADR_REQ_GAMMA)}) {
                const int rc = adr_credit_subbook_ladders_host(
                    method, K, P, times.data(), dfs.data(), jac.data(), (mask & ADR_REQ_GAMMA) ? hess.data() : nullptr, b.n(),
                    b.fix_off.data(), b.flt_off.data(), b.fix_tp.data(), b.fix_pay.data(), b.flt_tp.data(), b.flt_ts.data(),
                    b.flt_te.data(), b.flt_alpha.data(), nullptr, b.notional.data(), b.spread.data(), b.fix_sign.data(),
                    b.flt_sign.data(), b.z.data(), b.bucket.data(), b.fix_tau.data(), b.flt_tau.data(), G, B, sub_off.data(), mask,
                    out.data());
                expect(rc == ADR_OK, "a valid call");
                bool finite = true;
                for (double v : out) finite = finite && std::isfinite(v);
                expect(finite, "finite rows");
                expect(out[3 * (1 + Q + Q * Q)] == 0.0 && out[0] != 0.0, "an empty desk is zero, desk 0 is not");
            }
        if (G != 32) continue;
        // the refusals, each on a copy with one thing wrong
        auto call = [&](const Book& x, int g, const std::vector<int64_t>& off) {
            return adr_credit_subbook_ladders_host(ADR_INTERP_LINEAR_ZERO_RATES, K, P, times.data(), dfs.data(), jac.data(), hess.data(),
                                                   x.n(), x.fix_off.data(), x.flt_off.data(), x.fix_tp.data(), x.fix_pay.data(),
                                                   x.flt_tp.data(), x.flt_ts.data(), x.flt_te.data(), x.flt_alpha.data(), nullptr,
                                                   x.notional.data(), x.spread.data(), x.fix_sign.data(), x.flt_sign.data(), x.z.data(),
                                                   x.bucket.data(), x.fix_tau.data(), x.flt_tau.data(), g, B, off.data(), 7, out.data());
        };
        Book x = b;
        x.z[3] = NAN;
        expect(call(x, G, sub_off) == ADR_ERR_INVALID, "non-finite z");
        x = b; x.fix_tau[2] = INFINITY;
        expect(call(x, G, sub_off) == ADR_ERR_INVALID, "non-finite fixed spread time");
        x = b; x.flt_tau[7] = NAN;
        expect(call(x, G, sub_off) == ADR_ERR_INVALID, "non-finite float spread time");
        x = b; x.bucket[4] = -2;
        expect(call(x, G, sub_off) == ADR_ERR_INVALID, "bucket below -1");
        x = b; x.bucket[6] = G;
        expect(call(x, G, sub_off) == ADR_ERR_INVALID, "bucket at G");
        expect(call(b, 33, sub_off) == ADR_ERR_INVALID && call(b, -1, sub_off) == ADR_ERR_INVALID, "G outside 0 .. 32");
        x = b; x.bucket[sub_off[5] + 100] = 0;
        expect(call(x, G, sub_off) == ADR_ERR_INVALID && std::strstr(adr_last_error(), "not ordered by bucket"), "a desk not ordered by bucket");
        x = b; x.flt_tp[x.flt_off[1] + 1] += 2.0 / 365.0;
        expect(call(x, G, sub_off) == ADR_ERR_UNSUPPORTED && std::strstr(adr_last_error(), "trade 1 has a ratio node"), "a ratio node");
        std::vector<int64_t> bad = sub_off;
        bad[2] = bad[1] - 1;
        expect(call(b, G, bad) == ADR_ERR_INVALID, "decreasing sub_off");
    }
    std::printf(failures ? "%d check(s) failed\n" : "all checks passed\n", failures);
    return failures ? 1 : 0;
}
