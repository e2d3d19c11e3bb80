// Delta-gamma P&L of desk ladders under a scenario set (adr_ladder_pnl*; declarations, summation orders and the bit
// contract: include/adrates.h):
//     pnl[b][s] = delta_b . x_s + 1/2 x_s' Gamma_b x_s
// from the rows [pv, delta[P], gamma[P][P]] that adr_subbook_ladders* and adr_price's agg write.
//
// Layout: lane = scenario.  A block is kWaves waves of ONE group of 64 scenarios, whose shocks sit in LDS as
// x[p / 2][lane][p % 2] (512 P bytes: 16 KiB at P = 32, 128 KiB at P = 256); a lane reads two of its shocks with one
// ds_read_b128, 64 consecutive 16-byte slots over the wave, no bank conflict.  Every wave takes its own tile of kDesks
// desks and keeps their accumulators in registers, so ONE read of x[q] feeds kDesks fused multiply-adds: the CU issues
// about four wave-FMAs in the time of one 512-byte LDS read, and at kDesks = 8 the LDS pipe is a quarter as busy as the
// FMA pipe.  The ladder entries are the same for
// all 64 lanes (wave-uniform addresses from blockIdx and the wave's number): they come through the scalar data cache into
// SGPRs, one of which an FMA takes as an operand, so the Gamma stream costs neither VGPRs nor LDS bandwidth nor vector
// memory instructions.  A tile is taken once (the grid holds them all; no loop over tiles), every store comes after
// the tile's last load, and a store is 64 consecutive doubles of a row of [B][S].
//
// The host twin runs the same ladder_pnl_tile<1> per (desk, scenario).  Every step is an explicit fma(): one correctly
// rounded operation on either side, so device and twin agree bit for bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/adrates.h"
#include "blocking_call.hpp"
#include "host_pool.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: nothing is fused but the fma() calls written out below

namespace adr {
namespace lpnl {

constexpr int kWave = 64;
constexpr int kWaves = 8;           // waves of a block, all on one scenario group, each with its own desk tile
constexpr int kDesks = 8;           // desks per wave: the accumulators one read of x[q] feeds
constexpr int kThreads = kWave * kWaves;
constexpr int kUnroll = 4;          // columns of Gamma per step of the inner loop: kDesks * kUnroll doubles in SGPRs

// ------------------------------------------------------------------------------------------------ the sums (shared)
// For TD desks and ONE scenario x (x(p): its shock of pillar p), rows[d] a ladder row [pv, delta[P], gamma[P][P]]:
//     dl[d] = fma(delta_p, x_p, dl[d])                     p = 0 .. P - 1 in order, from +0.0
//     t_p   = fma(gamma_pq, x_q, t_p)                      q = 0 .. P - 1 in order, from +0.0
//     gm[d] = fma(t_p, x_p, gm[d])                         p = 0 .. P - 1 in order, from +0.0
// The pv slot is not read; gamma is used as given, row p times the shocks first.  Without kGamma gm stays +0.0.
template <int TD, bool kGamma, class X>
__host__ __device__ inline void ladder_pnl_tile(const double* const (&rows)[TD], int P, const X& x, double (&dl)[TD],
                                                double (&gm)[TD]) {
#pragma unroll
    for (int d = 0; d < TD; ++d) dl[d] = gm[d] = 0.0;
    for (int p = 0; p < P; ++p) {
        const double xp = x(p);
        if (kGamma) {
            double t[TD];
#pragma unroll
            for (int d = 0; d < TD; ++d) t[d] = 0.0;
            const int64_t row = 1 + P + static_cast<int64_t>(p) * P;
            int q = 0;
            for (; q + kUnroll <= P; q += kUnroll) {
                double xs[kUnroll];
                x.four(q, xs);
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
#pragma unroll
                    for (int d = 0; d < TD; ++d) t[d] = fma(rows[d][row + q + u], xs[u], t[d]);
                }
            }
            for (; q < P; ++q) {
                const double xq = x(q);
#pragma unroll
                for (int d = 0; d < TD; ++d) t[d] = fma(rows[d][row + q], xq, t[d]);
            }
#pragma unroll
            for (int d = 0; d < TD; ++d) gm[d] = fma(t[d], xp, gm[d]);
        }
#pragma unroll
        for (int d = 0; d < TD; ++d) dl[d] = fma(rows[d][1 + p], xp, dl[d]);
    }
}

// pnl_gamma = 1/2 gm (exact), pnl = dl + pnl_gamma: the parts add up to pnl bit for bit.
__host__ __device__ inline double gamma_part(double gm) { return 0.5 * gm; }
__host__ __device__ inline double total(double dl, double gm) { return dl + gamma_part(gm); }

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    const double* ladders;           // [B][1 + P + P P]
    const double* shocks;            // [S][P]
    double *pnl, *pnl_delta, *pnl_gamma;         // [B][S] each, or null
    int64_t B;
    int P, S;
};

// The group's shocks in LDS, two pillars of a lane side by side: x[p / 2][lane][p % 2], so that a lane's four shocks
// q .. q + 3 (q a multiple of 4) are two 16-byte reads, each of them 64 consecutive slots over the wave.
__host__ __device__ inline int lds_slot(int p, int lane) { return ((p >> 1) * kWave + lane) * 2 + (p & 1); }
inline size_t lds_bytes(int P) { return static_cast<size_t>((P + 1) / 2) * kWave * 2 * sizeof(double); }

struct LdsX {
    const double* p;                 // &x[0][lane][0]
    __device__ double operator()(int k) const { return p[lds_slot(k, 0)]; }
    __device__ void four(int q, double (&xs)[kUnroll]) const {
        const double2 lo = *reinterpret_cast<const double2*>(p + lds_slot(q, 0));
        const double2 hi = *reinterpret_cast<const double2*>(p + lds_slot(q + 2, 0));
        xs[0] = lo.x; xs[1] = lo.y; xs[2] = hi.x; xs[3] = hi.y;
    }
};
static_assert(kUnroll == 4, "LdsX::four reads two pairs");

template <bool kGamma>
__global__ __launch_bounds__(kThreads) void ladder_pnl_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) double s_x[];         // [ceil(P / 2)][64][2]: lds_slot
    const int P = a.P;
    const int64_t s0 = static_cast<int64_t>(blockIdx.y) * kWave;
    for (int i = threadIdx.x; i < P * kWave; i += kThreads) {
        const int l = i / P, p = i - l * P;              // consecutive threads read consecutive doubles of the rows
        const int64_t s = s0 + l < a.S ? s0 + l : a.S - 1;         // lanes beyond the set hold a copy of its last row
        s_x[lds_slot(p, l)] = a.shocks[s * P + p];
    }
    __syncthreads();

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b0 = (static_cast<int64_t>(blockIdx.x) * kWaves + wave) * kDesks;
    if (b0 >= a.B) return;
    const int nd = a.B - b0 < kDesks ? static_cast<int>(a.B - b0) : kDesks;
    const int64_t stride = 1 + P + static_cast<int64_t>(P) * P;
    const double* rows[kDesks];
#pragma unroll
    for (int d = 0; d < kDesks; ++d) rows[d] = a.ladders + (b0 + (d < nd ? d : 0)) * stride;      // uniform: scalar loads
    double dl[kDesks], gm[kDesks];
    ladder_pnl_tile<kDesks, kGamma>(rows, P, LdsX{s_x + lds_slot(0, lane)}, dl, gm);

    const int64_t s = s0 + lane;
    if (s >= a.S) return;
#pragma unroll
    for (int d = 0; d < kDesks; ++d) {
        if (d >= nd) break;
        const int64_t o = (b0 + d) * a.S + s;
        if (kGamma && a.pnl) a.pnl[o] = total(dl[d], gm[d]);
        if (a.pnl_delta) a.pnl_delta[o] = dl[d];
        if (kGamma && a.pnl_gamma) a.pnl_gamma[o] = gamma_part(gm[d]);
    }
}

// -------------------------------------------------------------------------------------------------------------- host
struct HostX {
    const double* p;                 // the scenario's row of shocks
    double operator()(int k) const { return p[k]; }
    void four(int q, double (&xs)[kUnroll]) const {
        for (int u = 0; u < kUnroll; ++u) xs[u] = p[q + u];
    }
};

// The scalar checks of every entry.  B = 0 asks for nothing and is no error: the caller returns after them.
int check(const std::string& w, int64_t B, int P, const double* ladders, int S, const double* shocks, const double* pnl,
          const double* pnl_delta, const double* pnl_gamma) {
    if (B < 0 || S < 1 || P < 1) return adr_set_error(ADR_ERR_INVALID, w + ": B >= 0, S >= 1 and P >= 1 are needed");
    if (P > ADR_LADDER_PNL_MAX_PILLARS)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": " + std::to_string(P) + " pillars; at most ADR_LADDER_PNL_MAX_PILLARS (256), "
                                                      "whose 64 scenarios of shocks fit the LDS of a CU");
    if (!shocks || (B > 0 && !ladders)) return adr_set_error(ADR_ERR_INVALID, w + ": ladders / shocks_bp is NULL");
    if (!pnl && !pnl_delta && !pnl_gamma) return adr_set_error(ADR_ERR_INVALID, w + ": no output asked for (pnl, pnl_delta and pnl_gamma are all NULL)");
    return ADR_OK;
}

// The launch on `stream`; every pointer is device memory, B >= 1.
int enqueue(const std::string& w, const Args& a, hipStream_t stream) {
    const int64_t groups = (static_cast<int64_t>(a.S) + kWave - 1) / kWave;
    const int64_t tiles = (a.B + kDesks - 1) / kDesks, bx = (tiles + kWaves - 1) / kWaves;
    if (groups > 65535) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": more than 65535 * 64 scenarios in one launch");
    if (bx * kThreads > INT32_MAX) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": more than 2^31 / 8 desks in one launch");
    const bool gamma = a.pnl || a.pnl_gamma;
    auto kernel = gamma ? &ladder_pnl_kernel<true> : &ladder_pnl_kernel<false>;
    const size_t lds = lds_bytes(a.P);
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       static_cast<int>(lds));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(bx), static_cast<unsigned>(groups)), dim3(kThreads), lds, stream, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

}  // namespace lpnl
}  // namespace adr

namespace LP = adr::lpnl;

extern "C" {

int adr_ladder_pnl_dev(adr_ctx* ctx, int64_t B, int P, const double* ladders_dev, int S, const double* shocks_bp_dev, double* pnl_dev,
                       double* pnl_delta_dev, double* pnl_gamma_dev, void* stream) {
    const std::string w = "adr_ladder_pnl_dev";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = LP::check(w, B, P, ladders_dev, S, shocks_bp_dev, pnl_dev, pnl_delta_dev, pnl_gamma_dev);
    if (rc != ADR_OK || B == 0) return rc;
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    return LP::enqueue(w, LP::Args{ladders_dev, shocks_bp_dev, pnl_dev, pnl_delta_dev, pnl_gamma_dev, B, P, S}, st);
}

int adr_ladder_pnl(adr_ctx* ctx, int64_t B, int P, const double* ladders, int S, const double* shocks_bp, double* pnl,
                   double* pnl_delta, double* pnl_gamma) {
    const std::string w = "adr_ladder_pnl";
    if (!ctx) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx");
    int rc = LP::check(w, B, P, ladders, S, shocks_bp, pnl, pnl_delta, pnl_gamma);
    if (rc != ADR_OK || B == 0) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const size_t n_out = static_cast<size_t>(B) * S;
    double *dlad, *dx, *dpnl, *ddelta, *dgamma;
    adr::call::Staging mem;
    mem.in(&dlad, ladders, static_cast<size_t>(B) * (1 + P + static_cast<size_t>(P) * P));
    mem.in(&dx, shocks_bp, static_cast<size_t>(S) * P);
    mem.out(&dpnl, pnl, n_out, pnl != nullptr);                     // the outputs asked for
    mem.out(&ddelta, pnl_delta, n_out, pnl_delta != nullptr);
    mem.out(&dgamma, pnl_gamma, n_out, pnl_gamma != nullptr);
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) rc = LP::enqueue(w, LP::Args{dlad, dx, dpnl, ddelta, dgamma, B, P, S}, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_ladder_pnl_host(int64_t B, int P, const double* ladders, int S, const double* shocks_bp, double* pnl, double* pnl_delta,
                        double* pnl_gamma) {
    const std::string w = "adr_ladder_pnl_host";
    const int rc = LP::check(w, B, P, ladders, S, shocks_bp, pnl, pnl_delta, pnl_gamma);
    if (rc != ADR_OK || B == 0) return rc;
    const bool gamma = pnl || pnl_gamma;
    const int64_t stride = 1 + P + static_cast<int64_t>(P) * P;
    // a thread per 2^22 terms or so
    const int64_t grain = std::max<int64_t>(1, (int64_t(1) << 22) / (static_cast<int64_t>(S) * P * P));
    adr::parallel_ranges(B, adr::pool_threads(B, grain), [&](int, int64_t lo, int64_t hi) {
        for (int64_t b = lo; b < hi; ++b)
            for (int64_t s = 0; s < S; ++s) {
                const double* const rows[1] = {ladders + b * stride};
                const LP::HostX x{shocks_bp + s * P};
                double dl[1], gm[1];
                if (gamma) LP::ladder_pnl_tile<1, true>(rows, P, x, dl, gm);
                else LP::ladder_pnl_tile<1, false>(rows, P, x, dl, gm);
                const int64_t o = b * S + s;
                if (pnl) pnl[o] = LP::total(dl[0], gm[0]);
                if (pnl_delta) pnl_delta[o] = dl[0];
                if (pnl_gamma) pnl_gamma[o] = LP::gamma_part(gm[0]);
            }
    });
    return ADR_OK;
}

}  // extern "C"
