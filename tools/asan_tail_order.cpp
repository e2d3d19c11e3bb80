// Stand-alone sanitizer driver for adr_scenario_tail_order_host, adr_scenario_tail_alloc_select_host, adr_scenario_total_host,
// adr_shock_gather_host and adr_tail_components_host (CPU only; not a test of the suite and not for a GPU machine): calls
// the host twins on exactly sized heap buffers - rows of 1, 2, 17, 8 193 and 40 000 P&L values with base_col = -1, the
// first and the last column and k = 1 and the largest tail; tie rows whose k-th value lies inside a run of equal values,
// checked for the lowest indices; a NaN row; matrices of 1, 65 and 130 rows through the allocation; the gather with a
// negative and an out-of-range index - and over the refusals.  Build the library's sources and this file with
// -fsanitize=address,undefined on the host side and run it:
//   make -C adrates_amd/csrc OBJDIR=build_asan OUT=build_asan/libadrates_asan.so EXTRA="-Xarch_host -fsanitize=address,undefined"
//   clang++ -std=c++17 -g -fsanitize=address,undefined -Iinclude tools/asan_tail_order.cpp \
//           -Ladrates_amd/csrc/build_asan -ladrates_asan -Wl,-rpath,$PWD/adrates_amd/csrc/build_asan -o build_asan/driver
//   ASAN_OPTIONS=detect_leaks=0 build_asan/driver      (the HIP runtime the library links keeps its start-up allocations)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "adrates.h"

int main() {
    int failed = 0;
    auto expect = [&](int64_t got, int64_t want, const char* what) {
        if (got != want) {
            std::printf("%s: %lld, expected %lld\n", what, static_cast<long long>(got), static_cast<long long>(want));
            ++failed;
        }
    };
    for (int m : {1, 2, 17, 8193, 40000})
        for (int base : {-1, 0, m})
            for (int k : {1, m < ADR_SCENARIO_ALLOC_MAX ? m : ADR_SCENARIO_ALLOC_MAX}) {
                const int B = 3, width = base < 0 ? m : m + 1;
                std::vector<double> rows(static_cast<size_t>(B) * width), var(B), es(B);
                std::vector<int64_t> order(static_cast<size_t>(B) * k);
                for (size_t i = 0; i < rows.size(); ++i) rows[i] = std::sin(0.37 * static_cast<double>(i)) * 100.0;
                expect(adr_scenario_tail_order_host(B, width, rows.data(), base, k, order.data(), var.data(), es.data()), ADR_OK,
                       "adr_scenario_tail_order_host");
                for (int64_t e : order)
                    if (e < 0 || e >= m) expect(e, 0, "an index outside the row");
            }

    // ties: 9.0 everywhere, 3.25 on every third index, two values of -2.25; k = 50 takes the two and the 48 lowest ties
    {
        const int m = 20000, k = 50;
        std::vector<double> rows(static_cast<size_t>(2) * m, 9.0), var(2), es(2);
        for (int e = 1; e < m; e += 3) rows[e] = 3.25;
        rows[17000] = rows[3] = -2.25;
        rows[m + 5] = NAN;                                           // the second row holds a NaN
        std::vector<int64_t> order(static_cast<size_t>(2) * k);
        expect(adr_scenario_tail_order_host(2, m, rows.data(), -1, k, order.data(), var.data(), es.data()), ADR_OK, "ties");
        expect(order[0], 3, "ties: the first index");
        expect(order[1], 17000, "ties: the second index");
        for (int i = 2; i < k; ++i) expect(order[i], 1 + 3 * (i - 2), "ties: the lowest indices of the run, in order");
        expect(var[0] == -3.25 && es[0] == -(2 * -2.25 + 48 * 3.25) / 50.0 ? 1 : 0, 1, "ties: var and es");
        for (int i = 0; i < k; ++i) expect(order[k + i], -1, "a NaN row: index -1");
        expect(var[1] != var[1] && es[1] != es[1] ? 1 : 0, 1, "a NaN row: NaN figures");
        std::vector<double> equal(m, 3.25);                         // k_rem = k: the first k indices
        expect(adr_scenario_tail_order_host(1, m, equal.data(), -1, k, order.data(), var.data(), es.data()), ADR_OK, "equal values");
        for (int i = 0; i < k; ++i) expect(order[i], i, "equal values: the first k indices");
    }

    for (int B : {1, 65, 130})
        for (int m : {100, 8193})
            for (int base : {-1, m}) {
                const int width = base < 0 ? m : m + 1, k = m / 50;
                std::vector<double> rows(static_cast<size_t>(B) * width), tot(m), cv(B), ce(B), cv2(B), ce2(B);
                double var = 0.0, es = 0.0, var2 = 0.0, es2 = 0.0;
                for (size_t i = 0; i < rows.size(); ++i) rows[i] = std::sin(0.37 * static_cast<double>(i)) * 100.0;
                expect(adr_scenario_tail_alloc_select_host(B, width, rows.data(), base, k, &var, &es, cv.data(), ce.data()), ADR_OK,
                       "adr_scenario_tail_alloc_select_host");
                expect(adr_scenario_total_host(B, width, rows.data(), base, tot.data()), ADR_OK, "adr_scenario_total_host");
                if (m <= ADR_SCENARIO_ALLOC_MAX) {
                    expect(adr_scenario_tail_alloc_host(B, width, rows.data(), base, k, &var2, &es2, cv2.data(), ce2.data()), ADR_OK,
                           "adr_scenario_tail_alloc_host");
                    expect(var == var2 && es == es2 && cv == cv2 && ce == ce2 ? 1 : 0, 1, "the allocation's bits");
                }
            }

    {
        const int S = 40, P = 3, k = 5;
        std::vector<double> shocks(static_cast<size_t>(S) * P), out(static_cast<size_t>(k) * P), cv(2), ce(2);
        for (size_t i = 0; i < shocks.size(); ++i) shocks[i] = static_cast<double>(i);
        std::vector<int64_t> order{39, 0, 40, 7, 7};
        expect(adr_shock_gather_host(k, P, shocks.data(), S, order.data(), out.data()), ADR_OK, "adr_shock_gather_host");
        expect(out[0] == 117.0 && out[5] == 2.0 && out[6] != out[6] && out[9] == 21.0 ? 1 : 0, 1, "the gathered rows");
        order[0] = -1;
        expect(adr_shock_gather_host(k, P, shocks.data(), S, order.data(), out.data()), ADR_OK, "adr_shock_gather_host, NaN");
        for (double v : out) expect(v != v ? 1 : 0, 1, "a negative first index: NaN rows");
        expect(adr_tail_components_host(2, k, shocks.data(), cv.data(), ce.data()), ADR_OK, "adr_tail_components_host");
        expect(cv[0] == -4.0 && ce[0] == -2.0 && cv[1] == -9.0 && ce[1] == -7.0 ? 1 : 0, 1, "the components");
        expect(adr_shock_gather_host(0, P, shocks.data(), S, order.data(), out.data()), ADR_ERR_INVALID, "k < 1");
        expect(adr_shock_gather_host(k, 257, shocks.data(), S, order.data(), out.data()), ADR_ERR_INVALID, "P > 256");
        expect(adr_shock_gather_host(k, P, shocks.data(), S, nullptr, out.data()), ADR_ERR_INVALID, "NULL order");
        expect(adr_tail_components_host(0, k, shocks.data(), cv.data(), ce.data()), ADR_ERR_INVALID, "B < 1");
        expect(adr_tail_components_host(2, k, nullptr, cv.data(), ce.data()), ADR_ERR_INVALID, "NULL pnl");
    }

    std::vector<double> rows(2 * 20000, 0.0), out(2);
    std::vector<int64_t> order(2 * 8193);
    expect(adr_scenario_tail_order_host(2, 20000, rows.data(), -1, 8193, order.data(), out.data(), out.data()), ADR_ERR_UNSUPPORTED,
           "k > 8192");
    expect(adr_scenario_tail_order_host(2, 20000, rows.data(), -1, 0, order.data(), out.data(), out.data()), ADR_ERR_INVALID, "k < 1");
    expect(adr_scenario_tail_order_host(2, 20000, rows.data(), 0, 20000, order.data(), out.data(), out.data()), ADR_ERR_INVALID, "k > m");
    expect(adr_scenario_tail_order_host(2, 20000, rows.data(), 20000, 5, order.data(), out.data(), out.data()), ADR_ERR_INVALID, "base_col");
    expect(adr_scenario_tail_order_host(0, 20000, rows.data(), -1, 5, order.data(), out.data(), out.data()), ADR_ERR_INVALID, "B < 1");
    expect(adr_scenario_tail_order_host(2, 20000, rows.data(), -1, 5, nullptr, out.data(), out.data()), ADR_ERR_INVALID, "NULL order");
    expect(adr_scenario_tail_alloc_select_host(2, 20000, rows.data(), -1, 8193, out.data(), out.data(), out.data(), out.data()),
           ADR_ERR_UNSUPPORTED, "the allocation, k > 8192");
    expect(adr_scenario_tail_alloc_select_host(2, 20000, rows.data(), -1, 5, out.data(), out.data(), nullptr, out.data()), ADR_ERR_INVALID,
           "the allocation, NULL comp_var");
    expect(adr_scenario_total_host(2, 20000, rows.data(), 20000, out.data()), ADR_ERR_INVALID, "the totals, base_col");
    expect(adr_scenario_tail_order_work(1, 786432, 7865) > 0 ? 0 : 1, 0, "adr_scenario_tail_order_work");
    expect(adr_scenario_tail_order_work(1, 1048576, 10486), 0, "adr_scenario_tail_order_work beyond the limit");
    expect(adr_scenario_tail_alloc_select_work(1000, 262144, 2622) > 0 ? 0 : 1, 0, "adr_scenario_tail_alloc_select_work");
    std::printf(failed ? "%d checks failed\n" : "all calls returned as expected\n", failed);
    return failed ? 1 : 0;
}
