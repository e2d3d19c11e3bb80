// Discount factors of shocked curves, values only (adr_curve_dfs_shocked*; the contract: include/adrates.h): the scan of
// bootstrap_kernel (curve_build.hip) and build_engine_curve (market/curves/curve_tables.py) without its derivatives,
//     r_p  = base_rates[p] + shocks_bp[s][p] * 1e-4
//     v    = 1 + r a_i ;  Pp = 0 <= prev_idx[i] < i ? pv01[prev_idx[i]] : 0 ;  r = r_{pillar[i]}
//     d_i  = prev_idx[i] >= 0 ? (1 - r Pp) / v : 1 / v ;  pv01[i] = Pp + a_i d_i
// for S shock rows where adr_shock_normal_dev left them, into dfs[S][K], which is all the scenario kernels read.
// Contraction is off and there is no libm call: every entry has the bits of the host builder at the rates r, hence those
// of adr_curve_set_build's discount factors.
//
// Layout: lane = scenario, a wave = 64 consecutive scenarios, and the waves of a block share nothing.  acc, pillar and
// prev_idx are the same for all lanes (wave-uniform addresses: scalar loads).  A lane needs its own rates and its own
// pv01 of any earlier knot: both live scenario-minor in work_dev, rates[P][S] then pv01[K][S], so the 64 lanes of a
// wave read and write 512 contiguous bytes; a lane reads only what it wrote itself, so no barrier orders them.  One
// state path, in global memory: [K][64] doubles of LDS would hold one wave per CU at K = 264 and none at K = 1 242.
// Both ends are scenario-major - a lane's shock row lies 8 ld bytes from its neighbour's, its dfs row 8 K bytes - so both
// go through the wave's LDS tile stage[64][kRun | 1] (rows padded to an odd count of doubles: the 64-bit accesses of 32
// lanes fall on 64 distinct banks): the wave loads kRun columns of its 64 shock rows and stores kRun knots of its 64
// dfs rows in the order of memory, runs of 8 kRun = 128 bytes, a cache line; four waves' tiles are 34 KiB of a block's LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "blocking_call.hpp"
#include "host_pool.hpp"

#pragma clang fp contract(off)      // the IEEE operations of the host builder, in its order

// what this file needs of an adr_curve_plan: its owner and the scan arrays on the device (capi.hip)
int adr_curve_plan_scan_view(const adr_curve_plan* plan, const adr_ctx** owner, int* K, int* P, const double** acc_dev,
                             const int32_t** pillar_dev, const int32_t** prev_idx_dev);

namespace adr {
namespace cdfs {

constexpr int kWave = 64;
constexpr int kWaves = 4;           // waves of a block, each with its own 64 scenarios
constexpr int kRun = 16;            // columns of the shock rows, and knots of the dfs rows, per transpose step
constexpr int kRow = kRun | 1;      // doubles per row of the tile

// ------------------------------------------------------------------------------------------------ the scan (shared)
__host__ __device__ inline double shocked_rate(double base, double shock_bp) { return base + shock_bp * 1e-4; }

// One knot: the discount factor; *pv01 is the knot's PV01.  `Pp`: the predecessor's PV01, 0.0 where it has none to read.
__host__ __device__ inline double knot_df(double r, double a, int prev, double Pp, double* pv01) {
    const double v = 1.0 + r * a;
    const double d = prev >= 0 ? (1.0 - r * Pp) / v : 1.0 / v;
    *pv01 = Pp + a * d;
    return d;
}

__host__ __device__ inline bool bad_df(double d) { return !(d > 0.0) || !(d < INFINITY); }

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    const double* acc;               // [K]
    const int32_t* pillar;           // [K]
    const int32_t* prev_idx;         // [K]
    const double* base;              // [P]
    const double* shocks;            // [S][ld]
    double* dfs;                     // [S][K]
    int32_t* bad;                    // [S] or null
    double* work;                    // rates[P][S], then pv01[K][S]
    int K, P, S, ld;
};

// Element e of a run of n columns of the wave's 64 rows in the order of memory: row e / n, column e % n.
__global__ __launch_bounds__(kWave * kWaves) void curve_dfs_kernel(Args a) {
    __shared__ double s_stage[kWaves][kWave * kRow];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* st = s_stage[wave];
    const int64_t S = a.S, s0 = (static_cast<int64_t>(blockIdx.x) * kWaves + wave) * kWave, s = s0 + lane;
    const bool live = s < S;         // the others meet the barriers and touch no memory
    double* rates = a.work;
    double* pv = a.work + static_cast<int64_t>(a.P) * S;

    for (int p0 = 0; p0 < a.P; p0 += kRun) {
        const int pn = a.P - p0 < kRun ? a.P - p0 : kRun;
        for (int e = lane; e < kWave * pn; e += kWave) {
            const int r = e / pn, c = e - r * pn;
            if (s0 + r < S) st[r * kRow + c] = a.shocks[(s0 + r) * a.ld + p0 + c];
        }
        __syncthreads();
        if (live)
            for (int c = 0; c < pn; ++c) rates[(p0 + c) * S + s] = shocked_rate(a.base[p0 + c], st[lane * kRow + c]);
        __syncthreads();
    }

    bool bad = false;
    for (int k0 = 0; k0 < a.K; k0 += kRun) {
        const int kn = a.K - k0 < kRun ? a.K - k0 : kRun;
        if (live)
            for (int c = 0; c < kn; ++c) {
                const int i = k0 + c, prev = a.prev_idx[i];
                const double Pp = prev >= 0 && prev < i ? pv[prev * S + s] : 0.0;
                double pv01;
                const double d = knot_df(rates[a.pillar[i] * S + s], a.acc[i], prev, Pp, &pv01);
                pv[i * S + s] = pv01;
                st[lane * kRow + c] = d;
                bad = bad || bad_df(d);
            }
        __syncthreads();
        for (int e = lane; e < kWave * kn; e += kWave) {
            const int r = e / kn, c = e - r * kn;
            if (s0 + r < S) a.dfs[(s0 + r) * a.K + k0 + c] = st[r * kRow + c];
        }
        __syncthreads();
    }
    if (live && a.bad) a.bad[s] = bad ? 1 : 0;
}

// -------------------------------------------------------------------------------------------------------------- host
int check(const std::string& w, int P, int S, int ld, const void* base, const void* shocks, const void* dfs) {
    if (S < 1) return adr_set_error(ADR_ERR_INVALID, w + ": S >= 1 is needed");
    if (ld < P) return adr_set_error(ADR_ERR_INVALID, w + ": a row stride of " + std::to_string(ld) + " for " + std::to_string(P) + " pillars; ld >= P is needed");
    if (!base || !shocks || !dfs) return adr_set_error(ADR_ERR_INVALID, w + ": base_rates / shocks_bp / dfs is NULL");
    return ADR_OK;
}

int check_base(const std::string& w, int P, const double* base) {
    for (int p = 0; p < P; ++p)
        if (!std::isfinite(base[p])) return adr_set_error(ADR_ERR_INVALID, w + ": base rates must be finite");
    return ADR_OK;
}

// The plan's scan for a call on `ctx`.
int plan_args(const std::string& w, const adr_ctx* ctx, const adr_curve_plan* plan, Args* a) {
    if (!ctx || !plan) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx / plan");
    const adr_ctx* owner = nullptr;
    const int rc = adr_curve_plan_scan_view(plan, &owner, &a->K, &a->P, &a->acc, &a->pillar, &a->prev_idx);
    if (rc != ADR_OK) return rc;
    if (owner != ctx) return adr_set_error(ADR_ERR_INVALID, w + ": the plan was created through another ctx");
    return ADR_OK;
}

// The launch on `stream`; every pointer is device memory.
int enqueue(const std::string& w, const Args& a, hipStream_t stream) {
    const int64_t blocks = (static_cast<int64_t>(a.S) + kWave * kWaves - 1) / (kWave * kWaves);
    hipLaunchKernelGGL(curve_dfs_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kWave * kWaves), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

}  // namespace cdfs
}  // namespace adr

namespace CD = adr::cdfs;

extern "C" {

int64_t adr_curve_dfs_shocked_work(const adr_curve_plan* plan, int S) {
    const adr_ctx* owner = nullptr;
    CD::Args a{};
    if (!plan || S < 1 || adr_curve_plan_scan_view(plan, &owner, &a.K, &a.P, &a.acc, &a.pillar, &a.prev_idx) != ADR_OK) return 0;
    return (static_cast<int64_t>(a.K) + a.P) * S;
}

int adr_curve_dfs_shocked_dev(adr_ctx* ctx, const adr_curve_plan* plan, const double* base_rates_dev, int S, int ld,
                              const double* shocks_bp_dev, double* dfs_dev, int32_t* bad_dev, double* work_dev, void* stream) {
    const std::string w = "adr_curve_dfs_shocked_dev";
    CD::Args a{};
    int rc = CD::plan_args(w, ctx, plan, &a);
    if (rc == ADR_OK) rc = CD::check(w, a.P, S, ld, base_rates_dev, shocks_bp_dev, dfs_dev);
    if (rc != ADR_OK) return rc;
    if (!work_dev) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_curve_dfs_shocked_work doubles are needed)");
    hipStream_t st = nullptr;
    rc = adr::call::target_stream(w, ctx, static_cast<hipStream_t>(stream), &st);
    if (rc != ADR_OK) return rc;
    a.base = base_rates_dev; a.shocks = shocks_bp_dev; a.dfs = dfs_dev; a.bad = bad_dev; a.work = work_dev;
    a.S = S; a.ld = ld;
    return CD::enqueue(w, a, st);
}

int adr_curve_dfs_shocked(adr_ctx* ctx, const adr_curve_plan* plan, const double* base_rates, int S, int ld, const double* shocks_bp,
                          double* dfs, int32_t* bad) {
    const std::string w = "adr_curve_dfs_shocked";
    CD::Args a{};
    int rc = CD::plan_args(w, ctx, plan, &a);
    if (rc == ADR_OK) rc = CD::check(w, a.P, S, ld, base_rates, shocks_bp, dfs);
    if (rc == ADR_OK) rc = CD::check_base(w, a.P, base_rates);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    double *d_base, *d_x, *d_df, *d_w;
    int32_t* d_bad;
    adr::call::Staging mem;
    mem.in(&d_base, base_rates, a.P);
    mem.in(&d_x, shocks_bp, static_cast<size_t>(S) * ld);
    mem.out(&d_df, dfs, static_cast<size_t>(S) * a.K);
    mem.scratch(&d_w, static_cast<size_t>(a.K + a.P) * S);
    if (bad) mem.out(&d_bad, bad, S);
    else mem.scratch(&d_bad, S);                    // the kernel writes the flags whether or not they are asked for
    const hipError_t e = mem.begin(stream);
    a.base = d_base; a.shocks = d_x; a.dfs = d_df; a.bad = d_bad; a.work = d_w;
    a.S = S; a.ld = ld;
    if (e == hipSuccess) rc = CD::enqueue(w, a, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_curve_dfs_shocked_host(int K, int P, const double* acc, const int32_t* pillar, const int32_t* prev_idx, const double* base_rates,
                               int S, int ld, const double* shocks_bp, double* dfs, int32_t* bad) {
    const std::string w = "adr_curve_dfs_shocked_host";
    if (K < 1 || P < 1) return adr_set_error(ADR_ERR_INVALID, w + ": K >= 1 and P >= 1 are needed");
    if (!acc || !pillar || !prev_idx) return adr_set_error(ADR_ERR_INVALID, w + ": null scan arrays");
    int rc = CD::check(w, P, S, ld, base_rates, shocks_bp, dfs);
    if (rc == ADR_OK) rc = CD::check_base(w, P, base_rates);
    if (rc != ADR_OK) return rc;
    for (int i = 0; i < K; ++i) {
        if (pillar[i] < 0 || pillar[i] >= P) return adr_set_error(ADR_ERR_INVALID, w + ": pillar index out of range");
        if (prev_idx[i] < -1 || prev_idx[i] >= K) return adr_set_error(ADR_ERR_INVALID, w + ": prev_idx out of range");
    }
    // a thread per 2^16 knots or so
    const int64_t grain = std::max<int64_t>(1, (int64_t(1) << 16) / K);
    adr::parallel_ranges(S, adr::pool_threads(S, grain), [&](int, int64_t lo, int64_t hi) {
        std::vector<double> rates(static_cast<size_t>(P)), pv(static_cast<size_t>(K));
        for (int64_t s = lo; s < hi; ++s) {
            for (int p = 0; p < P; ++p) rates[p] = CD::shocked_rate(base_rates[p], shocks_bp[s * ld + p]);
            bool any = false;
            for (int i = 0; i < K; ++i) {
                const int prev = prev_idx[i];
                const double d = CD::knot_df(rates[pillar[i]], acc[i], prev, prev >= 0 && prev < i ? pv[prev] : 0.0, &pv[i]);
                dfs[s * K + i] = d;
                any = any || CD::bad_df(d);
            }
            if (bad) bad[s] = any ? 1 : 0;
        }
    });
    return ADR_OK;
}

}  // extern "C"
