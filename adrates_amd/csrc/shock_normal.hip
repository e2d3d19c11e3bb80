// Correlated normal shocks from a factor matrix (adr_shock_normal*; the generator, the order of the products and the
// contract: include/adrates.h):
//     x[s][p] = sum_j factor[p][j] z[s][j]
// with z from Philox4x32-10 and Box-Muller, a pure function of (seed, global scenario index, j).
//
// Layout: lane = scenario, a wave = 64 consecutive scenarios, and the waves of a block share nothing.  A lane draws its
// F normals pair by pair (one Philox call gives the cosine and the sine of a pair) into the wave's LDS as
// z[j / 2][lane][j % 2] - ladder_pnl.hip's layout of its shocks: the pair goes in with one 16-byte store and four
// normals come back with two ds_read_b128, 64 consecutive 16-byte slots over the wave, no bank conflict.  That is
// 1024 ceil(F / 2) bytes per wave, 128 KiB at F = 256, so the block is sized to it: as many waves as fit, four at the
// most.  The products run over a tile of kPillars pillars whose accumulators are registers, so ONE read of z[j] feeds
// kPillars fused multiply-adds; the factor entries are the same for all lanes (wave-uniform addresses) and come through
// the scalar data cache into SGPRs.  A lane holds a ROW of the output, 8 P bytes apart from its neighbour's, so the
// tile goes through an LDS transpose: kStage (64; 32 when F > 192 leaves no room for more) pillars of the 64 scenarios
// are staged as stage[lane][pillar], rows padded to an odd count of doubles (the stores of 16 lanes then fall on 16
// distinct bank pairs), and the wave stores them in the order of memory: whole rows of [S][P] when P <= 64 - the
// wave's 64 P doubles are ONE run -, runs of kStage doubles (512 or 256 bytes) otherwise.
//
// The host twin runs the same functions per scenario.  u is exact on both sides; log, sqrt, sin and cos are each
// library's, so z and x agree with the twin to a few ulp, not bit for bit (the tests hold both to a 50-digit reference).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "blocking_call.hpp"
#include "host_pool.hpp"

#pragma clang fp contract(off)      // as ladder_pnl.hip: nothing is fused but the fma() calls written out below

namespace adr {
namespace shock {

constexpr int kWave = 64;
constexpr int kMaxWaves = 4;        // waves of a block, each with its own 64 scenarios
constexpr int kPillars = 8;         // pillars per tile: the accumulators one read of z[j] feeds
constexpr int kUnroll = 4;          // normals per step of the inner loop
constexpr int kStage = 64;          // pillars per transpose step
constexpr int kStageSmall = 32;     // ... when the normals leave less than 64 x 65 doubles of a wave's LDS
constexpr size_t kLdsBudget = 160 * 1024;

// ---------------------------------------------------------------------------------------------- generator (shared)
struct Words {
    uint32_t w[4];
};

__host__ __device__ inline uint32_t mulhi32(uint32_t a, uint32_t b) {
    return static_cast<uint32_t>((static_cast<uint64_t>(a) * b) >> 32);
}

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC11).
__host__ __device__ inline Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(M0, c0), lo0 = M0 * c0, hi1 = mulhi32(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return Words{{c0, c1, c2, c3}};
}

// The words of normals 2 i and 2 i + 1 of generating scenario g.
__host__ __device__ inline Words pair_words(uint64_t seed, uint64_t g, uint32_t i) {
    return philox4x32_10(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), i, 0u, static_cast<uint32_t>(seed),
                         static_cast<uint32_t>(seed >> 32));
}

// (((hi << 32 | lo) >> 11) + 0.5) 2^-53: the 53-bit integer is exact, the sum is rounded once (to nearest even, which
// matters from 2^52 on) and the scaling is exact.  In (0, 1]; never 0.
__host__ __device__ inline double uniform_of(uint32_t lo, uint32_t hi) {
    const uint64_t n = ((static_cast<uint64_t>(hi) << 32) | lo) >> 11;
    return (static_cast<double>(n) + 0.5) * 0x1p-53;
}

// Box-Muller: z0 = r cos(2 pi u2), z1 = r sin(2 pi u2), r = sqrt(-2 log(u1)).
__host__ __device__ inline void normal_pair(const Words& w, double* z0, double* z1) {
    const double u1 = uniform_of(w.w[0], w.w[1]), u2 = uniform_of(w.w[2], w.w[3]);
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586476925286766559 * u2;
    *z0 = r * cos(a);
    *z1 = r * sin(a);
}

// The generating scenario of global row gi and whether the row is the negated one of its pair.
__host__ __device__ inline uint64_t generating(int64_t gi, int antithetic, bool* negate) {
    *negate = antithetic && (gi & 1);
    return static_cast<uint64_t>(antithetic ? gi >> 1 : gi);
}

// ------------------------------------------------------------------------------------------------ the sums (shared)
// For TP pillars and ONE scenario (z(j): its normal j), rows[i] row p_i of the factor matrix:
//     x[i] = fma(factor[p_i][j], z_j, x[i])                j = 0 .. F - 1 in order, from +0.0
template <int TP, class Z>
__host__ __device__ inline void shock_tile(const double* const (&rows)[TP], int F, const Z& z, double (&x)[TP]) {
#pragma unroll
    for (int i = 0; i < TP; ++i) x[i] = 0.0;
    int j = 0;
    for (; j + kUnroll <= F; j += kUnroll) {
        double zs[kUnroll];
        z.four(j, zs);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
            for (int i = 0; i < TP; ++i) x[i] = fma(rows[i][j + u], zs[u], x[i]);
        }
    }
    for (; j < F; ++j) {
        const double zj = z(j);
#pragma unroll
        for (int i = 0; i < TP; ++i) x[i] = fma(rows[i][j], zj, x[i]);
    }
}

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    uint64_t seed;
    int64_t first;
    const double* factor;            // [P][F]
    double* out;                     // [S][P]
    int S, P, F, antithetic;
};

// A wave's normals, two of a lane side by side: z[j / 2][lane][j % 2].
__host__ __device__ inline int z_slot(int j, int lane) { return ((j >> 1) * kWave + lane) * 2 + (j & 1); }
inline size_t z_doubles(int F) { return static_cast<size_t>((F + 1) / 2) * kWave * 2; }
inline int stage_pillars(int P, int F) { return std::min(P, F > 192 ? kStageSmall : kStage); }
__host__ __device__ inline int stage_row(int pc) { return pc | 1; }      // odd: 16 lanes' stores fall on 16 distinct bank pairs
inline size_t wave_doubles(int P, int F) { return z_doubles(F) + static_cast<size_t>(kWave) * stage_row(stage_pillars(P, F)); }
inline int block_waves(int P, int F) {
    return static_cast<int>(std::max<size_t>(1, std::min<size_t>(kMaxWaves, kLdsBudget / (wave_doubles(P, F) * sizeof(double)))));
}

struct LdsZ {
    const double* p;                 // &z[0][lane][0]
    __device__ double operator()(int j) const { return p[z_slot(j, 0)]; }
    __device__ void four(int j, double (&zs)[kUnroll]) const {
        const double2 lo = *reinterpret_cast<const double2*>(p + z_slot(j, 0));
        const double2 hi = *reinterpret_cast<const double2*>(p + z_slot(j + 2, 0));
        zs[0] = lo.x; zs[1] = lo.y; zs[2] = hi.x; zs[3] = hi.y;
    }
};
static_assert(kUnroll == 4, "LdsZ::four reads two pairs");

// blockDim.x = 64 x the block's waves; per wave wave_d doubles of LDS: the normals, then stage[64][pc | 1].
__global__ __launch_bounds__(kWave * kMaxWaves) void shock_normal_kernel(Args a, int wave_d, int z_d, int pc) {
    extern __shared__ __attribute__((aligned(16))) double s_shock[];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves = blockDim.x >> 6;
    double* zw = s_shock + static_cast<size_t>(wave) * wave_d;
    double* st = zw + z_d;
    const int P = a.P, F = a.F;
    const int64_t s0 = (static_cast<int64_t>(blockIdx.x) * waves + wave) * kWave;        // may lie beyond S: nothing stored
    // lanes beyond the set draw a copy of its last row (every wave of the block meets every barrier below)
    const int64_t s = s0 + lane < a.S ? s0 + lane : a.S - 1;
    bool negate;
    const uint64_t g = generating(a.first + s, a.antithetic, &negate);
    for (int i = 0; 2 * i < F; ++i) {
        double2 z;
        normal_pair(pair_words(a.seed, g, static_cast<uint32_t>(i)), &z.x, &z.y);
        *reinterpret_cast<double2*>(zw + z_slot(2 * i, lane)) = z;      // the lane's own slots: no barrier before it reads them
    }
    const int row = stage_row(pc);
    for (int p0 = 0; p0 < P; p0 += pc) {
        const int pn = P - p0 < pc ? P - p0 : pc;
        for (int pt = 0; pt < pn; pt += kPillars) {
            const double* rows[kPillars];
#pragma unroll
            for (int i = 0; i < kPillars; ++i) rows[i] = a.factor + static_cast<int64_t>(p0 + (pt + i < pn ? pt + i : pt)) * F;   // uniform: scalar loads
            double x[kPillars];
            shock_tile<kPillars>(rows, F, LdsZ{zw + z_slot(0, lane)}, x);
#pragma unroll
            for (int i = 0; i < kPillars; ++i)
                if (pt + i < pn) st[lane * row + pt + i] = negate ? -x[i] : x[i];
        }
        __syncthreads();
        // the staged pn pillars of 64 scenarios in the order of memory: element e is scenario e / pn, pillar e % pn
        for (int e = lane; e < kWave * pn; e += kWave) {
            const int r = e / pn, c = e - r * pn;
            if (s0 + r < a.S) a.out[(s0 + r) * P + p0 + c] = st[r * row + c];
        }
        __syncthreads();
    }
}

// The uniforms alone (the test hook adr_shock_uniforms): u[s][i][0 .. 1] of pair i of row s, one thread each.
__global__ __launch_bounds__(256) void shock_uniforms_kernel(uint64_t seed, int64_t first, int64_t S, int pairs, int antithetic,
                                                             double* u) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= S * pairs) return;
    const int64_t s = t / pairs;
    bool negate;
    const Words w = pair_words(seed, generating(first + s, antithetic, &negate), static_cast<uint32_t>(t - s * pairs));
    u[2 * t] = uniform_of(w.w[0], w.w[1]);
    u[2 * t + 1] = uniform_of(w.w[2], w.w[3]);
}

// -------------------------------------------------------------------------------------------------------------- host
struct HostZ {
    const double* p;                 // the scenario's normals
    double operator()(int j) const { return p[j]; }
    void four(int j, double (&zs)[kUnroll]) const {
        for (int u = 0; u < kUnroll; ++u) zs[u] = p[j + u];
    }
};

// The scalar checks of every entry.
int check(const std::string& w, int64_t first, int S, int P, int F, const double* factor, int antithetic, const double* out) {
    if (S < 1 || P < 1 || F < 1) return adr_set_error(ADR_ERR_INVALID, w + ": S >= 1, P >= 1 and F >= 1 are needed");
    if (F > P) return adr_set_error(ADR_ERR_INVALID, w + ": " + std::to_string(F) + " factors for " + std::to_string(P) + " pillars; F <= P is needed");
    if (P > ADR_LADDER_PNL_MAX_PILLARS)
        return adr_set_error(ADR_ERR_INVALID, w + ": " + std::to_string(P) + " pillars; at most ADR_LADDER_PNL_MAX_PILLARS (256), as "
                                                  "adr_ladder_pnl takes");
    if (first < 0 || first > INT64_MAX - S) return adr_set_error(ADR_ERR_INVALID, w + ": first_scenario must be >= 0 and first_scenario + S fit an int64");
    if (antithetic != 0 && antithetic != 1) return adr_set_error(ADR_ERR_INVALID, w + ": antithetic must be 0 or 1");
    if (!factor || !out) return adr_set_error(ADR_ERR_INVALID, w + ": factor / out is NULL");
    return ADR_OK;
}

// The launch on `stream`; every pointer is device memory.
int enqueue(const std::string& w, const Args& a, hipStream_t stream) {
    const int waves = block_waves(a.P, a.F), pc = stage_pillars(a.P, a.F);
    const size_t wave_d = wave_doubles(a.P, a.F), lds = wave_d * waves * sizeof(double);
    const int64_t groups = (static_cast<int64_t>(a.S) + kWave - 1) / kWave, blocks = (groups + waves - 1) / waves;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&shock_normal_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(shock_normal_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kWave * waves), lds, stream, a,
                           static_cast<int>(wave_d), static_cast<int>(z_doubles(a.F)), pc);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

}  // namespace shock
}  // namespace adr

namespace SN = adr::shock;

extern "C" {

int adr_shock_normal_dev(adr_ctx* ctx, uint64_t seed, int64_t first_scenario, int S, int P, int F, const double* factor_dev,
                         int antithetic, double* out_dev, void* stream) {
    const std::string w = "adr_shock_normal_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = SN::check(w, first_scenario, S, P, F, factor_dev, antithetic, out_dev);
    if (rc != ADR_OK) return rc;
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    return SN::enqueue(w, SN::Args{seed, first_scenario, factor_dev, out_dev, S, P, F, antithetic}, st);
}

int adr_shock_normal(adr_ctx* ctx, uint64_t seed, int64_t first_scenario, int S, int P, int F, const double* factor, int antithetic,
                     double* out) {
    const std::string w = "adr_shock_normal";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = SN::check(w, first_scenario, S, P, F, factor, antithetic, out);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *dfac, *dx;
    adr::call::Staging mem;
    mem.in(&dfac, factor, static_cast<size_t>(P) * F);
    mem.out(&dx, out, static_cast<size_t>(S) * P);
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) rc = SN::enqueue(w, SN::Args{seed, first_scenario, dfac, dx, S, P, F, antithetic}, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_shock_normal_host(uint64_t seed, int64_t first_scenario, int S, int P, int F, const double* factor, int antithetic,
                          double* out) {
    const std::string w = "adr_shock_normal_host";
    const int rc = SN::check(w, first_scenario, S, P, F, factor, antithetic, out);
    if (rc != ADR_OK) return rc;
    // a thread per 2^20 products or so
    const int64_t grain = std::max<int64_t>(1, (int64_t(1) << 20) / (static_cast<int64_t>(P) * F + 64 * F));
    adr::parallel_ranges(S, adr::pool_threads(S, grain), [&](int, int64_t lo, int64_t hi) {
        std::vector<double> z(static_cast<size_t>(F) + 1);
        for (int64_t s = lo; s < hi; ++s) {
            bool negate;
            const uint64_t g = SN::generating(first_scenario + s, antithetic, &negate);
            for (int i = 0; 2 * i < F; ++i) SN::normal_pair(SN::pair_words(seed, g, static_cast<uint32_t>(i)), &z[2 * i], &z[2 * i + 1]);
            for (int p = 0; p < P; ++p) {
                const double* const rows[1] = {factor + static_cast<int64_t>(p) * F};
                double x[1];
                SN::shock_tile<1>(rows, F, SN::HostZ{z.data()}, x);
                out[s * P + p] = negate ? -x[0] : x[0];
            }
        }
    });
    return ADR_OK;
}

void adr_shock_words_host(const uint32_t counter[4], const uint32_t key[2], uint32_t words[4]) {
    const SN::Words w = SN::philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
    for (int i = 0; i < 4; ++i) words[i] = w.w[i];
}

int adr_shock_uniforms_host(uint64_t seed, int64_t first_scenario, int S, int F, int antithetic, double* u) {
    const std::string w = "adr_shock_uniforms_host";
    if (S < 1 || F < 1 || first_scenario < 0 || first_scenario > INT64_MAX - S || !u || (antithetic != 0 && antithetic != 1))
        return adr_set_error(ADR_ERR_INVALID, w + ": S >= 1, F >= 1, first_scenario >= 0, antithetic 0 / 1 and u are needed");
    const int pairs = (F + 1) / 2;
    for (int64_t s = 0; s < S; ++s) {
        bool negate;
        const uint64_t g = SN::generating(first_scenario + s, antithetic, &negate);
        for (int i = 0; i < pairs; ++i) {
            const SN::Words wd = SN::pair_words(seed, g, static_cast<uint32_t>(i));
            u[2 * (s * pairs + i)] = SN::uniform_of(wd.w[0], wd.w[1]);
            u[2 * (s * pairs + i) + 1] = SN::uniform_of(wd.w[2], wd.w[3]);
        }
    }
    return ADR_OK;
}

int adr_shock_uniforms(adr_ctx* ctx, uint64_t seed, int64_t first_scenario, int S, int F, int antithetic, double* u) {
    const std::string w = "adr_shock_uniforms";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    if (S < 1 || F < 1 || first_scenario < 0 || first_scenario > INT64_MAX - S || !u || (antithetic != 0 && antithetic != 1))
        return adr_set_error(ADR_ERR_INVALID, w + ": S >= 1, F >= 1, first_scenario >= 0, antithetic 0 / 1 and u are needed");
    hipStream_t stream = nullptr;
    const int rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const int pairs = (F + 1) / 2;
    const int64_t n = static_cast<int64_t>(S) * pairs, blocks = (n + 255) / 256;
    if (blocks > INT32_MAX) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": more than 2^31 blocks of pairs");
    double* du;
    adr::call::Staging mem;
    mem.out(&du, u, static_cast<size_t>(n) * 2);
    hipError_t e = mem.begin(stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(SN::shock_uniforms_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, stream, seed, first_scenario,
                           static_cast<int64_t>(S), pairs, antithetic, du);
        e = hipGetLastError();
    }
    return mem.finish(w, ADR_OK, e, stream);
}

}  // extern "C"
