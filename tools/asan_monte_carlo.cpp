// Stand-alone sanitizer driver for adr_shock_normal_host, adr_shock_uniforms_host and adr_scenario_tail_select_host (CPU
// only; not a test of the suite and not for a GPU machine): calls the host twins on exactly sized heap buffers - factor
// matrices of 1 to 256 pillars with F = 1, P / 2 + 1 and P (odd F: the last sine is dropped), 1 and 65 scenarios, with
// and without the antithetic pairing; rows of 1, 2, 17, 16 385 and 40 000 P&L values with base_col = -1, the first and
// the last column and k = 1 and the largest tail - and over the refusals.  Build the library's sources and this file
// with -fsanitize=address,undefined on the host side and run it:
//   make -C adrates_amd/csrc OBJDIR=build_asan OUT=build_asan/libadrates_asan.so EXTRA="-Xarch_host -fsanitize=address,undefined"
//   clang++ -std=c++17 -g -fsanitize=address,undefined -Iinclude tools/asan_monte_carlo.cpp \
//           -Ladrates_amd/csrc/build_asan -ladrates_asan -Wl,-rpath,$PWD/adrates_amd/csrc/build_asan -o build_asan/driver
//   ASAN_OPTIONS=detect_leaks=0 build_asan/driver      (the HIP runtime the library links keeps its start-up allocations)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "adrates.h"

int main() {
    int failed = 0;
    auto expect = [&](int got, int want, const char* what) {
        if (got != want) {
            std::printf("%s: status %d, expected %d\n", what, got, want);
            ++failed;
        }
    };
    for (int P : {1, 2, 3, 33, 65, 256})
        for (int F : {1, P / 2 + 1, P})
            for (int S : {1, 65})
                for (int anti : {0, 1}) {
                    if (F > P) continue;
                    std::vector<double> factor(static_cast<size_t>(P) * F), out(static_cast<size_t>(S) * P);
                    for (size_t i = 0; i < factor.size(); ++i) factor[i] = std::cos(0.3 * static_cast<double>(i));
                    expect(adr_shock_normal_host(7, 3, S, P, F, factor.data(), anti, out.data()), ADR_OK, "adr_shock_normal_host");
                    std::vector<double> u(static_cast<size_t>(S) * ((F + 1) / 2) * 2);
                    expect(adr_shock_uniforms_host(7, 3, S, F, anti, u.data()), ADR_OK, "adr_shock_uniforms_host");
                }
    std::vector<double> one(4, 1.0);
    expect(adr_shock_normal_host(1, 0, 2, 1, 2, one.data(), 0, one.data()), ADR_ERR_INVALID, "F > P");
    expect(adr_shock_normal_host(1, -1, 2, 2, 2, one.data(), 0, one.data()), ADR_ERR_INVALID, "first_scenario < 0");
    expect(adr_shock_normal_host(1, 0, 0, 2, 2, one.data(), 0, one.data()), ADR_ERR_INVALID, "S < 1");
    expect(adr_shock_normal_host(1, 0, 2, 2, 2, nullptr, 0, one.data()), ADR_ERR_INVALID, "NULL factor");

    for (int m : {1, 2, 17, 16385, 40000})
        for (int base : {-1, 0, m})
            for (int k : {1, m < ADR_SCENARIO_TAIL_MAX ? m : ADR_SCENARIO_TAIL_MAX}) {
                const int B = 3, width = base < 0 ? m : m + 1;
                std::vector<double> rows(static_cast<size_t>(B) * width), var(B), es(B);
                for (size_t i = 0; i < rows.size(); ++i) rows[i] = std::sin(0.37 * static_cast<double>(i)) * 100.0;
                expect(adr_scenario_tail_select_host(B, width, rows.data(), base, k, var.data(), es.data()), ADR_OK,
                       "adr_scenario_tail_select_host");
            }
    std::vector<double> rows(2 * 20000, 0.0), out(2);
    expect(adr_scenario_tail_select_host(2, 20000, rows.data(), -1, 16385, out.data(), out.data()), ADR_ERR_UNSUPPORTED, "k > 16384");
    expect(adr_scenario_tail_select_host(2, 20000, rows.data(), -1, 0, out.data(), out.data()), ADR_ERR_INVALID, "k < 1");
    expect(adr_scenario_tail_select_host(2, 20000, rows.data(), 0, 20000, out.data(), out.data()), ADR_ERR_INVALID, "k > m");
    expect(adr_scenario_tail_select_host(2, 20000, rows.data(), 20000, 5, out.data(), out.data()), ADR_ERR_INVALID, "base_col");
    expect(adr_scenario_tail_select_work(1000, 262144, 2622) > 0 ? 0 : 1, 0, "adr_scenario_tail_select_work");
    std::printf(failed ? "%d calls failed\n" : "all calls returned as expected\n", failed);
    return failed ? 1 : 0;
}
