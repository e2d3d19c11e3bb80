// Year-on-year inflation swaps: projected amounts, inflation-leg PV and inflation-curve delta / gamma
// (adr_yoy_risk*; declarations and the input layout: include/adrates.h).
//
// The reference (cavour/market/position/engine.py:986-1353, `_compute_yoy_iis`) differentiates the YoY leg with jax
// with respect to the inflation curve's factors and chains the result through the Jacobian and Hessian of
// f_k = (1 + b_k)^T_k.  Both inflation schemes it can meet (LINEAR_ZERO_RATES, FLAT_FWD_RATES) make ln I(t) linear in
// the nodes' L_k = ln f_k = T_k ln(1 + b_k), with at most two knots of nonzero weight (simple_interp.hpp::log_weights).
// So per coupon 1 + y = I(te) / I(ts) = exp(sum_k c_k L_k), c = w(te) - w(ts) with at most 4 nonzero entries, and
//     dy / db_k          = (1 + y) c_k L'_k
//     d2y / db_k db_l    = (1 + y) (c_k c_l L'_k L'_l + [k == l] c_k L''_k),   L' = T / (1 + b), L'' = -T / (1 + b)^2,
// the reference's J^T H J + sum g * Hess in closed form.  Each coupon adds, with g = scale D(tp) / D(0) (1 + y), a
// rank-1 update of at most 4 x 4 entries plus a diagonal.  Knot 0 (t = 0, f = 1) has a zero Jacobian row and drops out.
//
// Layout: one wave (64 lanes) per block; a block prices ADR_YOY_CHUNK consecutive swaps one after the other.  The
// inflation nodes sit in LDS; the discount grid (up to 4096 knots) is read from global memory.  Per swap the lanes
// describe 64 coupons at a time in parallel (the lookups, exp, amount) and stage them in LDS; then the coupons are
// applied one by one in order: 16 lanes update the 4 x 4 block of the swap's LDS gamma, 4 lanes its delta, one lane its
// PV.  Every accumulator therefore sees its terms in coupon order; no atomics.  The swap's rows are stored with 64
// consecutive doubles per store instruction and, for the book, added to the block's chunk sums (registers), which a
// second kernel adds in a fixed order.  The host twin runs the same per-coupon code and the same orders.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "blocking_call.hpp"
#include "host_pool.hpp"
#include "simple_interp.hpp"
#include "yoy_nodes.hpp"

// The host and the device evaluate the same expressions; no contraction into fma, so the two differ only by their
// exp / log implementations.  The nodes, a coupon's description and its gamma entry are yoy_nodes.hpp's, shared with
// yoy_subbook_ladder.hip.
#pragma clang fp contract(off)

namespace adr {
namespace yoy {

constexpr int kWave = 64;                   // lanes per block
constexpr int kChunk = ADR_YOY_CHUNK;       // swaps per block
constexpr int kStage = 10;                  // staged doubles per coupon: u[4], v[4], g, pv
constexpr int kRedLanes = 64;               // the agg reduction's lanes per entry
constexpr int kRedEntries = 16;             // entries per reduction block
constexpr double kDeltaUnit = 1e-4, kGammaUnit = 1e-8;

struct Args {
    const double *dx, *dd;
    int K, dm;
    const double *T, *b;
    int P, im;
    int64_t n, m;
    const int64_t* off;
    const double* cpn;
    unsigned req;
    double *amount, *pv, *delta, *gamma, *work;
};

__host__ __device__ inline int64_t row_len(int P) { return 1 + P + static_cast<int64_t>(P) * P; }

inline size_t lds_bytes(int P) {
    return (4 * kNodes + static_cast<size_t>(P) * P + P + kStage * kWave) * sizeof(double) + 4 * kWave * sizeof(int);
}

// ------------------------------------------------------------------------------------------------------------ device
template <int kSlots>                       // kSlots * 64 >= P * P: the gamma entries a lane owns
__global__ __launch_bounds__(kWave) void yoy_risk_kernel(Args a) {
    extern __shared__ double lds[];
    const int P = a.P, PP = P * P, lane = threadIdx.x;
    double *s_x = lds, *s_L = s_x + kNodes, *s_L1 = s_L + kNodes, *s_L2 = s_L1 + kNodes;
    double *s_g = s_L2 + kNodes, *s_d = s_g + PP, *st = s_d + P;
    int* s_k = reinterpret_cast<int*>(st + kStage * kWave);
    for (int k = lane; k <= P; k += kWave) make_node(a.T, a.b, k, s_x + k, s_L + k, s_L1 + k, s_L2 + k);
    const double D0 = si::df(0.0, a.dx, a.dd, a.K, a.dm);
    __syncthreads();
    const Infl f{s_x, s_L, s_L1, s_L2, P + 1, a.im};
    const bool want_v = a.req & ADR_REQ_VALUE, want_d = a.req & ADR_REQ_DELTA, want_g = a.req & ADR_REQ_GAMMA;
    const bool per = a.req & ADR_YOY_PER_SWAP, agg = a.req & ADR_YOY_AGG;
    const bool rows = per || agg;
    double cg[kSlots];
#pragma unroll
    for (int j = 0; j < kSlots; ++j) cg[j] = 0.0;
    double cd = 0.0, cpv = 0.0;
    const int64_t first = static_cast<int64_t>(blockIdx.x) * kChunk;
    for (int s = 0; s < kChunk; ++s) {
        const int64_t sw = first + s;
        if (sw >= a.n) break;                               // uniform across the block
        for (int e = lane; e < PP; e += kWave) s_g[e] = 0.0;
        if (lane < P) s_d[lane] = 0.0;
        double pvacc = 0.0;                                 // lane 20's
        int64_t c0 = a.off[sw], c1 = a.off[sw + 1];
        if (c0 < 0 || c1 < c0 || c1 > a.m) {                // malformed offsets: no reads, a NaN PV
            c0 = c1 = 0;
            pvacc = NAN;
        }
        __syncthreads();
        for (int64_t base = c0; base < c1; base += kWave) {
            const int64_t i = base + lane;
            if (i < c1) {
                const Desc d = describe(a.dx, a.dd, a.K, a.dm, D0, f, a.cpn, a.m, i);
                if (a.amount) a.amount[i] = d.amount;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s_k[j * kWave + lane] = d.k[j];
                    st[j * kWave + lane] = d.u[j];
                    st[(4 + j) * kWave + lane] = d.v[j];
                }
                st[8 * kWave + lane] = d.g;
                st[9 * kWave + lane] = d.pv;
            }
            __syncthreads();
            if (rows) {
                const int cnt = static_cast<int>(c1 - base < kWave ? c1 - base : kWave);
                for (int j = 0; j < cnt; ++j) {
                    if (lane < 16) {
                        if (want_g) {
                            const int p = lane >> 2, q = lane & 3;
                            const int kp = s_k[p * kWave + j], kq = s_k[q * kWave + j];
                            if (kp > 0 && kq > 0) {
                                const double val = gamma_term(st[p * kWave + j], st[q * kWave + j], st[(4 + p) * kWave + j],
                                                              p == q);
                                double& e = s_g[(kp - 1) * P + (kq - 1)];
                                e = e + st[8 * kWave + j] * val;
                            }
                        }
                    } else if (lane < 20) {
                        const int p = lane - 16, kp = s_k[p * kWave + j];
                        if (kp > 0) {
                            double& e = s_d[kp - 1];
                            e = e + st[8 * kWave + j] * st[p * kWave + j];
                        }
                    } else if (lane == 20) {
                        pvacc = pvacc + st[9 * kWave + j];
                    }
                    __syncthreads();
                }
            }
            __syncthreads();
        }
        if (rows) {
            const double pv_s = __shfl(pvacc, 20);
            if (lane == 0) {
                if (per && want_v) a.pv[sw] = pv_s;
                cpv = cpv + pv_s;
            }
            if (lane < P) {
                const double dv = s_d[lane] * kDeltaUnit;
                if (per && want_d) a.delta[sw * P + lane] = dv;
                cd = cd + dv;
            }
            if (want_g) {
#pragma unroll
                for (int j = 0; j < kSlots; ++j) {
                    const int e = lane + j * kWave;
                    if (e < PP) {
                        const double gv = s_g[e] * kGammaUnit;
                        if (per) a.gamma[sw * PP + e] = gv;
                        cg[j] = cg[j] + gv;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (agg) {
        double* w = a.work + static_cast<int64_t>(blockIdx.x) * row_len(P);
        if (lane == 0) w[0] = want_v ? cpv : 0.0;
        if (lane < P) w[1 + lane] = want_d ? cd : 0.0;
#pragma unroll
        for (int j = 0; j < kSlots; ++j) {
            const int e = lane + j * kWave;
            if (e < PP) w[1 + P + e] = want_g ? cg[j] : 0.0;
        }
    }
}

// agg[e] = sum of the chunk rows' entry e: chunk j to lane j % 64 in order, then a fixed halving tree over the 64 lanes.
// The unrolled loop issues eight independent loads before it adds them in order.
__global__ __launch_bounds__(kRedLanes * kRedEntries) void yoy_agg_kernel(const double* work, int64_t chunks, int64_t R,
                                                                          double* agg) {
    __shared__ double s[kRedLanes][kRedEntries];
    const int ei = threadIdx.x % kRedEntries, cl = threadIdx.x / kRedEntries;
    const int64_t e = static_cast<int64_t>(blockIdx.x) * kRedEntries + ei;
    double acc = 0.0;
    if (e < R) {
#pragma unroll 8
        for (int64_t j = cl; j < chunks; j += kRedLanes) acc = acc + work[j * R + e];
    }
    s[cl][ei] = acc;
    __syncthreads();
    for (int h = kRedLanes / 2; h >= 1; h >>= 1) {
        if (cl < h) s[cl][ei] = s[cl][ei] + s[cl + h][ei];
        __syncthreads();
    }
    if (cl == 0 && e < R) agg[e] = s[0][ei];
}

// -------------------------------------------------------------------------------------------------------------- host
int validate(const char* who, int dm, int K, int im, int P, int64_t n, int64_t m, unsigned req, const void* times,
             const void* dfs, const void* T, const void* b, const void* off, const void* cpn, const void* pv,
             const void* delta, const void* gamma, const void* agg) {
    const std::string w(who);
    if (dm != ADR_INTERP_FLAT_FWD_RATES && dm != ADR_INTERP_LINEAR_FWD_RATES && dm != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": discount scheme must be FLAT_FWD_RATES (1), LINEAR_FWD_RATES (2) or "
                                                      "LINEAR_ZERO_RATES (4)");
    if (im != ADR_INTERP_FLAT_FWD_RATES && im != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": inflation scheme must be FLAT_FWD_RATES (1) or LINEAR_ZERO_RATES (4)");
    if (K < 2 || K > ADR_YOY_MAX_KNOTS)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": the discount grid needs 2 .. ADR_YOY_MAX_KNOTS (4096) knots");
    if (P < 1 || P > ADR_YOY_MAX_PILLARS)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": the inflation curve needs 1 .. ADR_YOY_MAX_PILLARS (64) pillars");
    if (!times || !dfs || !T || !b) return adr_set_error(ADR_ERR_INVALID, w + ": null curve arrays");
    if (n < 0 || m < 0 || (n > 0 && !off) || (m > 0 && !cpn)) return adr_set_error(ADR_ERR_INVALID, w + ": bad count / null array");
    const bool per = req & ADR_YOY_PER_SWAP, agg_on = req & ADR_YOY_AGG;
    if (per && n > 0 && (((req & ADR_REQ_VALUE) && !pv) || ((req & ADR_REQ_DELTA) && !delta) || ((req & ADR_REQ_GAMMA) && !gamma)))
        return adr_set_error(ADR_ERR_INVALID, w + ": a requested per-swap output is NULL");
    if (agg_on && !agg) return adr_set_error(ADR_ERR_INVALID, w + ": ADR_YOY_AGG without agg");
    return ADR_OK;
}

int check_host_arrays(const char* who, int K, const double* times, const double* dfs, int P, const double* T,
                      const double* b, int64_t n, int64_t m, const int64_t* off, const double* cpn) {
    const std::string w(who);
    for (int k = 0; k < K; ++k)
        if (!std::isfinite(times[k]) || !(dfs[k] > 0.0) || !std::isfinite(dfs[k]) || (k > 0 && times[k] < times[k - 1]))
            return adr_set_error(ADR_ERR_INVALID, w + ": knot times must be finite and non-decreasing, dfs positive");
    for (int k = 0; k < P; ++k)
        if (!std::isfinite(T[k]) || !std::isfinite(b[k]) || !(b[k] > -1.0) || !(T[k] > (k ? T[k - 1] : 0.0)))
            return adr_set_error(ADR_ERR_INVALID, w + ": pillar times must be increasing from > 0, rates finite and > -1");
    if (n == 0) return m == 0 ? ADR_OK : adr_set_error(ADR_ERR_INVALID, w + ": coupons without swaps");
    if (off[0] != 0 || off[n] != m) return adr_set_error(ADR_ERR_INVALID, w + ": cpn_off must run from 0 to m");
    for (int64_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return adr_set_error(ADR_ERR_INVALID, w + ": coupon offsets must be non-decreasing");
    for (int64_t i = 0; i < ADR_YOY_FIELDS * m; ++i)
        if (!std::isfinite(cpn[i])) return adr_set_error(ADR_ERR_INVALID, w + ": coupon fields must be finite");
    return ADR_OK;
}

// The reduction of yoy_agg_kernel on the host.
void reduce_chunks(const double* work, int64_t chunks, int64_t R, double* agg) {
    for (int64_t e = 0; e < R; ++e) {
        double p[kRedLanes];
        for (int cl = 0; cl < kRedLanes; ++cl) {
            p[cl] = 0.0;
            for (int64_t j = cl; j < chunks; j += kRedLanes) p[cl] = p[cl] + work[j * R + e];
        }
        for (int h = kRedLanes / 2; h >= 1; h >>= 1)
            for (int cl = 0; cl < h; ++cl) p[cl] = p[cl] + p[cl + h];
        agg[e] = p[0];
    }
}

template <int kSlots>
void launch(const Args& a, int64_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(yoy_risk_kernel<kSlots>, dim3(static_cast<unsigned>(blocks)), dim3(kWave), lds_bytes(a.P), stream, a);
}

}  // namespace yoy
}  // namespace adr

namespace Y = adr::yoy;

extern "C" {

int64_t adr_yoy_risk_work(int64_t n, int P) {
    if (n < 0 || P < 1 || P > ADR_YOY_MAX_PILLARS) return 0;
    return (n + Y::kChunk - 1) / Y::kChunk * Y::row_len(P);
}

int adr_yoy_risk_dev(adr_ctx* ctx, int disc_method, int K, const double* times, const double* dfs, int infl_method, int P,
                     const double* T, const double* b, int64_t n, int64_t m, const int64_t* cpn_off, const double* cpn,
                     uint32_t req_mask, double* amount, double* pv, double* delta, double* gamma, double* agg,
                     double* work, void* stream_v) {
    const char* who = "adr_yoy_risk_dev";
    int rc = Y::validate(who, disc_method, K, infl_method, P, n, m, req_mask, times, dfs, T, b, cpn_off, cpn, pv, delta,
                         gamma, agg);
    if (rc != ADR_OK) return rc;
    const bool agg_on = req_mask & ADR_YOY_AGG;
    if (agg_on && n > 0 && !work) return adr_set_error(ADR_ERR_INVALID, std::string(who) + ": ADR_YOY_AGG without work");
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(who, ctx, static_cast<hipStream_t>(stream_v), &stream);
    if (rc != ADR_OK) return rc;
    hipError_t e = hipSuccess;
    const int64_t blocks = (n + Y::kChunk - 1) / Y::kChunk;
    if (blocks > 0x7fffffff) return adr_set_error(ADR_ERR_UNSUPPORTED, std::string(who) + ": too many swaps for one launch");
    if (blocks > 0) {
        const Y::Args a{times, dfs, K, disc_method, T, b, P, infl_method, n, m, cpn_off, cpn,
                        req_mask, amount, pv, delta, gamma, work};
        if (P <= 8) Y::launch<1>(a, blocks, stream);
        else if (P <= 16) Y::launch<4>(a, blocks, stream);
        else if (P <= 32) Y::launch<16>(a, blocks, stream);
        else Y::launch<64>(a, blocks, stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess && agg_on) {
        const int64_t R = Y::row_len(P);
        hipLaunchKernelGGL(Y::yoy_agg_kernel, dim3(static_cast<unsigned>((R + Y::kRedEntries - 1) / Y::kRedEntries)),
                           dim3(Y::kRedLanes * Y::kRedEntries), 0, stream, work, blocks, R, agg);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return ADR_OK;
}

int adr_yoy_risk(adr_ctx* ctx, int disc_method, int K, const double* times, const double* dfs, int infl_method, int P,
                 const double* T, const double* b, int64_t n, int64_t m, const int64_t* cpn_off, const double* cpn,
                 uint32_t req_mask, double* amount, double* pv, double* delta, double* gamma, double* agg) {
    const char* who = "adr_yoy_risk";
    int rc = Y::validate(who, disc_method, K, infl_method, P, n, m, req_mask, times, dfs, T, b, cpn_off, cpn, pv, delta,
                         gamma, agg);
    if (rc == ADR_OK) rc = Y::check_host_arrays(who, K, times, dfs, P, T, b, n, m, cpn_off, cpn);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(who, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const bool per = req_mask & ADR_YOY_PER_SWAP, agg_on = req_mask & ADR_YOY_AGG;
    const bool wv = per && (req_mask & ADR_REQ_VALUE), wd = per && (req_mask & ADR_REQ_DELTA);
    const bool wg = per && (req_mask & ADR_REQ_GAMMA);
    const size_t PP = static_cast<size_t>(P) * P;
    double *dt, *ddf, *dT, *db, *dcpn, *damt, *dpv, *ddl, *dg, *dagg, *dwork;
    int64_t* doff;
    adr::call::Staging mem;
    mem.in(&dt, times, K);
    mem.in(&ddf, dfs, K);
    mem.in(&dT, T, P);
    mem.in(&db, b, P);
    mem.in(&dcpn, cpn, ADR_YOY_FIELDS * static_cast<size_t>(m));
    mem.in(&doff, cpn_off, n + 1, n > 0);           // null for an empty book
    mem.out(&damt, amount, m, amount != nullptr);
    mem.out(&dpv, pv, n, wv);
    mem.out(&ddl, delta, n * P, wd);
    mem.out(&dg, gamma, n * PP, wg);
    mem.out(&dagg, agg, Y::row_len(P), agg_on);
    mem.scratch(&dwork, adr_yoy_risk_work(n, P), agg_on);
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess)
        rc = adr_yoy_risk_dev(ctx, disc_method, K, dt, ddf, infl_method, P, dT, db, n, m, doff, dcpn, req_mask, damt, dpv, ddl, dg,
                              dagg, dwork, stream);
    return mem.finish(who, rc, e, stream);
}

int adr_yoy_risk_host(int disc_method, int K, const double* times, const double* dfs, int infl_method, int P,
                      const double* T, const double* b, int64_t n, int64_t m, const int64_t* cpn_off, const double* cpn,
                      uint32_t req_mask, double* amount, double* pv, double* delta, double* gamma, double* agg) {
    const char* who = "adr_yoy_risk_host";
    int rc = Y::validate(who, disc_method, K, infl_method, P, n, m, req_mask, times, dfs, T, b, cpn_off, cpn, pv, delta,
                         gamma, agg);
    if (rc == ADR_OK) rc = Y::check_host_arrays(who, K, times, dfs, P, T, b, n, m, cpn_off, cpn);
    if (rc != ADR_OK) return rc;
    const bool want_v = req_mask & ADR_REQ_VALUE, want_d = req_mask & ADR_REQ_DELTA, want_g = req_mask & ADR_REQ_GAMMA;
    const bool per = req_mask & ADR_YOY_PER_SWAP, agg_on = req_mask & ADR_YOY_AGG, rows = per || agg_on;
    const int PP = P * P;
    const int64_t R = Y::row_len(P), chunks = (n + Y::kChunk - 1) / Y::kChunk;
    double x[Y::kNodes], L[Y::kNodes], L1[Y::kNodes], L2[Y::kNodes];
    for (int k = 0; k <= P; ++k) Y::make_node(T, b, k, x + k, L + k, L1 + k, L2 + k);
    const Y::Infl f{x, L, L1, L2, P + 1, infl_method};
    const double D0 = adr::si::df(0.0, times, dfs, K, disc_method);
    std::vector<double> work(agg_on ? static_cast<size_t>(chunks * R) : 0, 0.0);
    adr::parallel_ranges(chunks, adr::pool_threads(chunks, 16), [&](int, int64_t lo, int64_t hi) {
        std::vector<double> g(PP), dl(P), cg(PP), cd(P);
        for (int64_t ch = lo; ch < hi; ++ch) {
            std::fill(cg.begin(), cg.end(), 0.0);
            std::fill(cd.begin(), cd.end(), 0.0);
            double cpv = 0.0;
            for (int64_t sw = ch * Y::kChunk; sw < std::min(n, (ch + 1) * Y::kChunk); ++sw) {
                std::fill(g.begin(), g.end(), 0.0);
                std::fill(dl.begin(), dl.end(), 0.0);
                double pvacc = 0.0;
                for (int64_t i = cpn_off[sw]; i < cpn_off[sw + 1]; ++i) {
                    const Y::Desc d = Y::describe(times, dfs, K, disc_method, D0, f, cpn, m, i);
                    if (amount) amount[i] = d.amount;
                    if (!rows) continue;
                    for (int p = 0; p < 4; ++p) {
                        if (d.k[p] <= 0) continue;
                        if (want_g)
                            for (int q = 0; q < 4; ++q)
                                if (d.k[q] > 0) {
                                    double& e = g[(d.k[p] - 1) * P + (d.k[q] - 1)];
                                    e = e + d.g * Y::gamma_term(d.u[p], d.u[q], d.v[p], p == q);
                                }
                        double& e = dl[d.k[p] - 1];
                        e = e + d.g * d.u[p];
                    }
                    pvacc = pvacc + d.pv;
                }
                if (!rows) continue;
                if (per && want_v) pv[sw] = pvacc;
                cpv = cpv + pvacc;
                for (int k = 0; k < P; ++k) {
                    const double dv = dl[k] * Y::kDeltaUnit;
                    if (per && want_d) delta[sw * P + k] = dv;
                    cd[k] = cd[k] + dv;
                }
                if (want_g)
                    for (int e = 0; e < PP; ++e) {
                        const double gv = g[e] * Y::kGammaUnit;
                        if (per) gamma[sw * PP + e] = gv;
                        cg[e] = cg[e] + gv;
                    }
            }
            if (agg_on) {
                double* w = work.data() + ch * R;
                w[0] = want_v ? cpv : 0.0;
                for (int k = 0; k < P; ++k) w[1 + k] = want_d ? cd[k] : 0.0;
                for (int e = 0; e < PP; ++e) w[1 + P + e] = want_g ? cg[e] : 0.0;
            }
        }
    });
    if (agg_on) Y::reduce_chunks(work.data(), chunks, R, agg);
    return ADR_OK;
}

}  // extern "C"
