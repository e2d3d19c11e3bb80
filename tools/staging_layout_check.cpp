// Stand-alone check of the blocking calls' memory plan (adrates_amd/csrc/staging_layout.hpp; CPU only, no HIP, not a test
// of the suite): every piece at a multiple of 16 bytes, no two overlapping, the total at the end of the last piece,
// absent pieces without room and null, mixed element types, and adr_yoy_risk's pieces with its outputs switched off.
// Build with the host compiler and the sanitizers, and run it:
//   c++ -std=c++17 -g -fsanitize=address,undefined -Iadrates_amd/csrc tools/staging_layout_check.cpp -o /tmp/staging_layout_check
//   /tmp/staging_layout_check
#include <cstdint>
#include <cstdio>
#include <vector>

#include "staging_layout.hpp"

using adr::call::StagingLayout;

static int failed = 0;
static void expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        ++failed;
    }
}

// Lays out `bytes` and checks the plan against a real buffer of the total: every present piece is written end to end
// (the address sanitizer sees a byte past the buffer), and no byte is written twice.
static StagingLayout check(const std::vector<size_t>& bytes) {
    StagingLayout l;
    std::vector<size_t> at;
    for (size_t b : bytes) at.push_back(l.add(b));
    std::vector<unsigned char> buf(l.total, 0);
    size_t end = 0;
    for (size_t i = 0; i < bytes.size(); ++i) {
        unsigned char* p = static_cast<unsigned char*>(StagingLayout::at(buf.data(), at[i]));
        if (bytes[i] == 0) {
            expect(at[i] == StagingLayout::kAbsent && p == nullptr, "an absent piece is null");
            continue;
        }
        expect(at[i] % StagingLayout::kAlign == 0, "a piece starts at a multiple of 16 bytes");
        expect(at[i] >= end && at[i] - end < StagingLayout::kAlign, "a piece starts at the first multiple of 16 after the last");
        for (size_t j = 0; j < bytes[i]; ++j) {
            expect(p[j] == 0, "no byte belongs to two pieces");
            p[j] = 1;
        }
        end = at[i] + bytes[i];
    }
    expect(l.total == end, "the total is the end of the last piece");
    return l;
}

int main() {
    expect(check({}).total == 0, "no piece, no bytes");
    expect(check({0, 0}).total == 0, "absent pieces alone take no room");
    expect(check({8}).total == 8, "one double");
    expect(check({8, 8}).total == 24, "the second double starts at 16");
    expect(check({0, 24, 0, 4, 0}).total == 36, "absent pieces between present ones take no room");
    // mixed types: doubles, int64 offsets, int32 flags, raw bytes
    check({5 * sizeof(double), 3 * sizeof(int64_t), 7 * sizeof(int32_t), 13, 1, 2 * sizeof(double)});
    // adr_scenario_tail at B = 3, S_tot = 130: the rows, var, es
    expect(check({3 * 130 * 8, 3 * 8, 3 * 8}).total == 3120 + 32 + 24, "adr_scenario_tail's three pieces");
    // adr_yoy_risk at K = 7, P = 5, n = 3 swaps, m = 11 coupons of 6 fields: times, dfs, T, b, cpn, cpn_off, then amount,
    // pv, delta, gamma, agg, work - everything on, then the outputs off one by one, then an empty book
    const size_t K = 7, P = 5, n = 3, m = 11, d = sizeof(double), R = 1 + P + P * P;
    const std::vector<size_t> in = {K * d, K * d, P * d, P * d, 6 * m * d, (n + 1) * sizeof(int64_t)};
    const std::vector<size_t> out = {m * d, n * d, n * P * d, n * P * P * d, R * d, R * d};
    for (unsigned off = 0; off < 64; ++off) {
        std::vector<size_t> pieces = in;
        size_t present = 0;
        for (size_t i = 0; i < out.size(); ++i) {
            pieces.push_back(off >> i & 1 ? 0 : out[i]);
            present += off >> i & 1 ? 0 : out[i];
        }
        const StagingLayout l = check(pieces);
        size_t least = present;
        for (size_t b : in) least += b;
        expect(l.total >= least && l.total < least + pieces.size() * StagingLayout::kAlign, "the padding is under 16 bytes a piece");
    }
    check({K * d, K * d, P * d, P * d, 0, 0, 0, 0, 0, 0, R * d, 0});
    std::printf(failed ? "%d checks failed\n" : "staging layout: all checks passed\n", failed);
    return failed ? 1 : 0;
}
