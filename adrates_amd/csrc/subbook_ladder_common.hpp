// What the sub-book ladder sources (subbook_ladder.hip, credit_subbook_ladder.hip and, for the curve block, the node's
// numbers, the cross sum and the launch, yoy_subbook_ladder.hip) have in common, once: the folding of a trade's cash flows
// into knot-space nodes, a node's lookup and its numbers, the projection of the curve block on the device and on the host,
// the owner search of the knot kernels, the knot launch, the checks of the handles and of the `_host` entries' arrays, the
// host's trade walk and the request and refusal wording.  These are what the host twins and the device are held to bit for
// bit and what decides a refusal's message, so a fix to any of them is made here.  A source keeps its knot kernel, its
// record layout, its entries and the order in which an entry calls the checks.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "curve_tables.hpp"
#include "host_pool.hpp"
#include "knot_tables.hpp"
#include "route.hpp"
#include "scenario_common.hpp"
#include "subbook.hpp"

const adr::CurveDev* adr_curve_device_view(const adr_curve* curve, const adr_ctx** owner);     // capi.hip
int64_t adr_trades_first_ratio(const adr_trades* trades);                                      // capi.hip

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace sbl {

using scen::DateW;
using scen::kChunk;
using scen::kWave;

constexpr int kMaxWaves = 16;
constexpr int kProjWaves = 8;       // waves of a projection block, each taking every eighth knot; summed in wave order
constexpr int kProjDesks = 8;       // sub-books per projection block

// ---------------------------------------------------------------------------------------------------- nodes (shared)
struct Flows {           // the cash-flow arrays of a batch
    const double *fix_tp, *fix_pay, *flt_tp, *flt_ts, *flt_te, *flt_alpha;
};

struct TradeRef {        // one trade
    int64_t f0, l0;      // its first fixed flow and float coupon
    int n_fix, n_flt;
    double notional, spread, fix_sign, flt_sign;
};

struct Amount {          // a node before its lookup: amount a at time t
    double t, a;
    bool on;
};

// Float coupon c of a trade without ratio nodes: N ((D(ts) / D(tp) - 1) + s alpha) D(tp) = N D(ts) + N (s alpha - 1) D(tp).
// The masks are the lite kernel's: a coupon counts when tp >= 0 and has no forward when alpha <= 0; the next coupon's
// start joins this payment node when it is the same date, and so does the fixed flow of the same index.
__host__ __device__ inline void float_nodes(const Flows& g, const TradeRef& r, int c, Amount* pay, Amount* start) {
    const int64_t i = r.l0 + c;
    const double tp = g.flt_tp[i], ts = g.flt_ts[i], al = g.flt_alpha[i];
    const bool valid = tp >= 0.0, accrues = al > 0.0;
    const double sn = r.flt_sign * r.notional;
    double a = valid ? sn * (r.spread * al - (accrues ? 1.0 : 0.0)) : 0.0;
    if (c + 1 < r.n_flt && g.flt_alpha[i + 1] > 0.0 && g.flt_tp[i + 1] >= 0.0 && g.flt_ts[i + 1] == tp) a = a + sn;
    if (c < r.n_fix) {
        const double xt = g.fix_tp[r.f0 + c];
        if (xt == tp && xt > 0.0) a = a + r.fix_sign * g.fix_pay[r.f0 + c];
    }
    pay->t = tp; pay->a = a; pay->on = a != 0.0;
    start->t = ts; start->a = sn;
    start->on = valid && accrues && !(c > 0 && g.flt_tp[i - 1] == ts);
}

// Fixed flow c: counts when tp > 0, unless it went with the float coupon of the same index.
__host__ __device__ inline Amount fixed_node(const Flows& g, const TradeRef& r, int c) {
    const double xt = g.fix_tp[r.f0 + c];
    const bool merged = c < r.n_flt && g.flt_tp[r.l0 + c] == xt;
    Amount n;
    n.t = xt;
    n.a = r.fix_sign * g.fix_pay[r.f0 + c];
    n.on = !merged && xt > 0.0 && n.a != 0.0;
    return n;
}

// The lookup of a date on the raw grid, its knots then renamed to the compact order.
template <bool kLog, class Comp>
__host__ __device__ inline DateW lookup(double t, const double* x, int K, int method, const Comp* compact_of) {
    DateW d = scen::date_weights<kLog>(t, x, K, method);
    d.a = compact_of[d.a];
    d.b = compact_of[d.b];
    return d;
}

struct Terms {           // what a node adds: pv, w at its two knots, D at its two knots, O at the first
    double pv, wa, wb, da, db, o;
};

struct Factor {          // a node's curve factor, which does not depend on its amount: exp(ba L[ka] + bb L[kb]) in ea, or
    double ea, eb;       // under LINEAR_FWD_RATES the two discount factors exp(L[ka]), exp(L[kb])
};

// L: ln d of the compact knots.
template <bool kLog>
__host__ __device__ inline Factor node_factor(const DateW& d, const double* L) {
    Factor f;
    const bool two = d.b != d.a;
    if (kLog) {
        double s = d.wa * L[d.a];
        if (two) s = s + d.wb * L[d.b];
        f.ea = exp(s);
        f.eb = 0.0;
    } else {
        f.ea = exp(L[d.a]);
        f.eb = two ? exp(L[d.b]) : 0.0;
    }
    return f;
}

// The node's numbers for one amount on a factor evaluated once (a node is linear in its amount in all three schemes).
template <bool kLog>
__host__ __device__ inline Terms node_terms_at(const DateW& d, double amount, const Factor& f) {
    Terms t;
    const bool two = d.b != d.a;
    if (kLog) {
        const double om = amount * f.ea;
        t.pv = om;
        t.wa = om * d.wa;
        t.wb = two ? om * d.wb : 0.0;
        t.da = t.wa * d.wa;
        t.db = t.wb * d.wb;
        t.o = two ? t.wa * d.wb : 0.0;
    } else {                 // D = d_a + w (d_b - d_a): the amounts on the two discount factors
        const double ca = two ? amount * (1.0 - d.wb) * f.ea : amount * f.ea;
        const double cb = two ? amount * d.wb * f.eb : 0.0;
        t.pv = ca + cb;
        t.wa = ca; t.wb = cb; t.da = ca; t.db = cb; t.o = 0.0;
    }
    return t;
}

// node_terms_at on node_factor in one expression, as subbook_ladder.hip has always formed it (the two give the same bits:
// the same products on the same exponentials).
template <bool kLog>
__host__ __device__ inline Terms node_terms(const DateW& d, double amount, const double* L) {
    Terms t;
    const bool two = d.b != d.a;
    if (kLog) {
        double s = d.wa * L[d.a];
        if (two) s = s + d.wb * L[d.b];
        const double om = amount * exp(s);
        t.pv = om;
        t.wa = om * d.wa;
        t.wb = two ? om * d.wb : 0.0;
        t.da = t.wa * d.wa;
        t.db = t.wb * d.wb;
        t.o = two ? t.wa * d.wb : 0.0;
    } else {                 // D = d_a + w (d_b - d_a): the amounts on the two discount factors
        const double ca = two ? amount * (1.0 - d.wb) * exp(L[d.a]) : amount * exp(L[d.a]);
        const double cb = two ? amount * d.wb * exp(L[d.b]) : 0.0;
        t.pv = ca + cb;
        t.wa = ca; t.wb = cb; t.da = ca; t.db = cb; t.o = 0.0;
    }
    return t;
}

// ----------------------------------------------------------------------------------------------- projection (shared)
// One knot's part of gamma[p][q]: a = LJ[k], b = LJ[k + 1] (read only where O_k is not zero), lc = LC[k][p][q].
__host__ __device__ inline double gamma_step(double s, double wk, double dk, double ok, double ap, double aq, double bp,
                                             double bq, double lc) {
    s = s + (dk * ap) * aq;
    if (ok != 0.0) s = s + ok * (ap * bq + bp * aq);
    if (wk != 0.0) s = s + wk * lc;
    return s;
}

__host__ __device__ inline double delta_step(double s, double wk, double aq) { return s + wk * aq; }

// One pillar's cross term of a second risk factor: sum_k wz_k LJ[k][p] over a knot-space table wz of mixed sums (the
// credit cells' spread table, the YoY desks' rows of M), the knots taken as the projection's waves take them.
template <class LJ>
__host__ __device__ inline double cross_sum(const double* wz, int Kc, const LJ& lj) {
    double tot = 0.0;
    for (int part = 0; part < kProjWaves; ++part) {
        double s = 0.0;
        for (int k = part; k < Kc; k += kProjWaves) s = delta_step(s, wz[k], lj(k));
        tot = part == 0 ? s : tot + s;
    }
    return tot;
}

// The curve block of out[b] = [pv, delta[Q], gamma[Q][Q]] from the desks' sums, the body of the two projection kernels.
// blockIdx.y < Q: row y of the gamma matrices (lane = column); blockIdx.y == Q: pv and the delta ladders.  A block takes
// kProjDesks desks, so a row of LJ / LC is read once for all of them.  kSpread: Q = P + a.G, and the rows and columns past
// the P pillars get +0.0 (credit_cell_kernel fills them); without it Q = P and the guards fold away.
template <bool kSpread, class Args>
__device__ inline void project_curve_block(const Args& a) {
    __shared__ int col_off[kWidePad + 1];
    __shared__ double s_part[kProjWaves][kProjDesks][kWave];
    const CurveDev& cv = a.cv;
    const int P = cv.P, Kc = cv.Kc;
    int Q = P;
    if constexpr (kSpread) Q = P + a.G;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b0 = static_cast<int64_t>(blockIdx.x) * kProjDesks;
    const int nd = a.B - b0 < kProjDesks ? static_cast<int>(a.B - b0) : kProjDesks;
    const int64_t stride = 1 + Q + static_cast<int64_t>(Q) * Q;
    const bool first = static_cast<int>(blockIdx.y) == Q;
    const int row = first ? 0 : blockIdx.y;
    const int p = !kSpread || row < P ? row : 0;
    if (threadIdx.x == 0) fill_col_off(col_off);
    __syncthreads();
    if (first && threadIdx.x < nd) a.out[(b0 + threadIdx.x) * stride] = a.sums[(b0 + threadIdx.x) * a.S];
    const bool wanted = (first ? a.want_delta != 0 : a.want_gamma != 0) && (!kSpread || row < P);
    double* dst = a.out + b0 * stride + (first ? 1 : 1 + Q + static_cast<int64_t>(row) * Q);
    for (int q0 = 0; q0 < Q; q0 += kWave) {              // columns in blocks of one wavefront
        const int q = q0 + lane, qq = q < P ? q : 0;     // lanes beyond the curve block compute a copy of column 0
        double s[kProjDesks];
#pragma unroll
        for (int d = 0; d < kProjDesks; ++d) s[d] = 0.0;
        if (wanted && (!kSpread || q0 < P)) {
            for (int k = wave; k < Kc; k += kProjWaves) {
                const double aq = lj_at(cv, k, qq);
                if (first) {
#pragma unroll
                    for (int d = 0; d < kProjDesks; ++d)
                        if (d < nd) s[d] = delta_step(s[d], a.sums[(b0 + d) * a.S + 1 + k], aq);
                    continue;
                }
                const bool next = k + 1 < Kc;
                const double ap = lj_at(cv, k, p);
                const double bp = next ? lj_at(cv, k + 1, p) : 0.0, bq = next ? lj_at(cv, k + 1, qq) : 0.0;
                const double lc = lc_at(cv, col_off, k, p, qq);
#pragma unroll
                for (int d = 0; d < kProjDesks; ++d)
                    if (d < nd) {
                        const double* rec = a.sums + (b0 + d) * a.S + 1 + k;           // uniform: scalar loads
                        s[d] = gamma_step(s[d], rec[0], rec[Kc], next ? rec[2 * Kc] : 0.0, ap, aq, bp, bq, lc);
                    }
            }
        }
#pragma unroll
        for (int d = 0; d < kProjDesks; ++d) s_part[wave][d][lane] = s[d];
        __syncthreads();
        if (wave == 0 && q < Q) {
            for (int d = 0; d < nd; ++d) {
                double t = s_part[0][d][lane];
#pragma unroll
                for (int i = 1; i < kProjWaves; ++i) t = t + s_part[i][d][lane];
                dst[d * stride + q] = !kSpread || q < P ? t * (first ? 1e-4 : 1e-8) : 0.0;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------------ device
// The wave's own LDS traffic in program order, for the compiler too.
__device__ inline void wave_lds_order() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The lane that holds the trade of flow f: the last lane j < cnt whose `begin` is <= f (the flows of a chunk are one
// contiguous run, so an empty trade shares its begin with its successor and never wins).  Every lane takes the six steps.
__device__ inline int owner_lane(int begin, int cnt, int f) {
    int pos = 0;
#pragma unroll
    for (int step = kWave / 2; step >= 1; step >>= 1) {
        const int cand = pos + step;
        const int v = __shfl(begin, cand & (kWave - 1), kWave);
        if (cand < cnt && v <= f) pos = cand;
    }
    return pos;
}

__device__ inline TradeRef owner_trade(const TradeHeader& h, int j) {
    TradeRef r;
    r.l0 = __shfl(h.flt_begin, j, kWave);
    r.f0 = __shfl(h.fix_begin, j, kWave);
    const int counts = __shfl(static_cast<int>(h.n_flt) | (static_cast<int>(h.n_fix) << 16), j, kWave);
    r.n_flt = counts & 0xffff;
    r.n_fix = counts >> 16;
    r.notional = __shfl(h.notional, j, kWave);
    r.spread = __shfl(h.spread, j, kWave);
    const int signs = __shfl((h.fix_sign < 0 ? 1 : 0) | (h.flt_sign < 0 ? 2 : 0), j, kWave);
    r.fix_sign = (signs & 1) ? -1.0 : 1.0;
    r.flt_sign = (signs & 2) ? -1.0 : 1.0;
    return r;
}

// -------------------------------------------------------------------------------------------------------------- host
// The knot times, ln d of the compact knots and the compact index every block of a knot kernel keeps in LDS.
inline size_t shared_bytes(int K, int Kc) { return (static_cast<size_t>(K) + Kc) * sizeof(double) + ((static_cast<size_t>(K) * sizeof(int16_t) + 7) & ~size_t(7)); }

// The waves of a block of a knot kernel with `tables` tables of Kc doubles per wave: as many as the LDS budget holds, 0
// when not even one fits.
inline int knot_waves(int K, int Kc, int tables) {
    const size_t per_wave = static_cast<size_t>(tables) * Kc * sizeof(double), shared = shared_bytes(K, Kc);
    if (shared + per_wave > scen::kLdsBudget) return 0;
    return static_cast<int>(std::min<size_t>(kMaxWaves, (scen::kLdsBudget - shared) / per_wave));
}

// A knot kernel's grid over `cap` chunks: its dynamic LDS, and at most two blocks per compute unit where two fit.
struct KnotGrid {
    int waves;
    size_t lds;
    unsigned blocks;
};
inline KnotGrid knot_grid(const adr_ctx* ctx, const CurveDev& cv, int tables, int64_t cap) {
    const int waves = knot_waves(cv.K, cv.Kc, tables);
    const size_t lds = shared_bytes(cv.K, cv.Kc) + static_cast<size_t>(waves) * tables * cv.Kc * sizeof(double);
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, static_cast<int64_t>(scen::kLdsBudget / lds)));
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((cap + waves - 1) / waves, per_cu * adr_ctx_compute_units(ctx)));
    return KnotGrid{waves, lds, static_cast<unsigned>(blocks)};
}

template <class Kernel, class Args>
hipError_t launch_knot(Kernel kernel, const Args& a, const KnotGrid& g, hipStream_t stream) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             static_cast<int>(g.lds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(kWave * g.waves), g.lds, stream, a);
    return hipGetLastError();
}

struct Request {
    bool delta, gamma;
};
inline Request request_of(uint32_t req_mask) {
    const bool gamma = (req_mask & ADR_REQ_GAMMA) != 0;
    return Request{gamma || (req_mask & ADR_REQ_DELTA) != 0, gamma};
}

inline std::string ratio_message(int64_t trade) {
    return ": trade " + std::to_string(trade) + " has a ratio node (a payment lag or a per-coupon notional); sub-book ladders "
           "take trades whose float coupons are paid on their accrual end";
}

// The first failing check decides an entry's message, so the checks come in pieces and each entry calls them in its own
// order, with its own between them.
// What an entry needs of its handles: present, of this ctx, with at least one sub-book and one trade.
struct Handles {
    const CurveDev* cv;
    const TradesDev* tr;
};
inline int check_handles(const std::string& w, const adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, int64_t B, Handles* h) {
    if (!ctx || !curve || !trades) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx/curve/trades");
    const adr_ctx *co = nullptr, *to = nullptr;
    h->cv = adr_curve_device_view(curve, &co);
    h->tr = adr_trades_device_view(trades, &to);
    if (co != ctx || to != ctx) return adr_set_error(ADR_ERR_INVALID, w + ": curve/trades were uploaded through another ctx");
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    if (h->tr->n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one trade is needed");
    return ADR_OK;
}

// ... and that the request can run on them: hess for GAMMA, one wave's tables in LDS, no ratio nodes.
inline int check_fit(const std::string& w, const adr_trades* trades, const Handles& h, const Request& rq, int tables) {
    if (rq.gamma && !h.cv->lc_lanes && !h.cv->lcflat)
        return adr_set_error(ADR_ERR_INVALID, w + ": GAMMA requested but the curve was uploaded without hess");
    if (knot_waves(h.cv->K, h.cv->Kc, tables) < 1)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": the knot tables of one wave (" + std::to_string(h.cv->Kc) +
                                                      " knots) do not fit the 160 KiB LDS of a CU");
    const int64_t ratio = adr_trades_first_ratio(trades);
    if (ratio >= 0) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ratio_message(ratio));
    return ADR_OK;
}

struct HostCurve {       // the curve as the _host entries take it
    int method, K, P;
    const double *times, *dfs, *jac, *hess;
};

// The checks of a _host entry, in three pieces: the scheme and the counts ...
inline int check_host_counts(const std::string& w, int method, int64_t n, int64_t B) {
    if (method != ADR_INTERP_FLAT_FWD_RATES && method != ADR_INTERP_LINEAR_FWD_RATES && method != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": only FLAT_FWD_RATES (1), LINEAR_FWD_RATES (2) and LINEAR_ZERO_RATES (4) "
                                                      "are implemented");
    if (n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one trade is needed");
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    return ADR_OK;
}

// ... the arrays that must be there ...
inline int check_host_arrays(const std::string& w, const HostCurve& c, const scen::HostBatch& b, const Request& rq, const double* out) {
    if (!out) return adr_set_error(ADR_ERR_INVALID, w + ": out is NULL");
    if (!c.times || !c.dfs || !c.jac) return adr_set_error(ADR_ERR_INVALID, w + ": null curve arrays");
    if (rq.gamma && !c.hess) return adr_set_error(ADR_ERR_INVALID, w + ": GAMMA requested but hess is NULL");
    if (!b.fix_off || !b.flt_off || !b.notional || !b.spread || !b.fix_sign || !b.flt_sign)
        return adr_set_error(ADR_ERR_INVALID, w + ": null per-trade array");
    return ADR_OK;
}

// ... and the trades, one by one - the first trade at fault decides the message - then their cash flows.
inline int check_host_trades(const std::string& w, const scen::HostBatch& b) {
    int rc = ADR_OK;
    for (int64_t i = 0; rc == ADR_OK && i < b.n; ++i) {
        rc = scen::check_leg_offsets(w, b, i, i + 1);
        if (rc == ADR_OK) rc = scen::check_trade_values(w, b, i, i + 1);
    }
    if (rc == ADR_OK) rc = scen::check_flows(w, b);
    return rc;
}

// After the entry's plan: the ratio refusal, then the curve's tables.
inline int host_tables(const std::string& w, const HostCurve& c, const scen::HostBatch& b, const Request& rq, CurveTables& t) {
    std::vector<uint8_t> ratio(static_cast<size_t>(b.n));
    route::flag_lagged(0, b.n, b.flt_off, b.flt_tp, b.flt_te, b.flt_alpha, b.flt_weight, ratio.data());
    const auto it = std::find(ratio.begin(), ratio.end(), uint8_t(1));
    if (it != ratio.end()) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ratio_message(it - ratio.begin()));
    const std::string err = build_curve_tables(c.K, c.P, c.times, c.dfs, c.jac, rq.gamma ? c.hess : nullptr, t);
    if (!err.empty()) return adr_set_error(ADR_ERR_INVALID, w + ": " + err);
    return ADR_OK;
}

// The trades of chunk ch on the host, in order: coupon(trade, i, c) for each float coupon of trade i, then fixed(trade, i, c)
// for each of its fixed flows.
template <class Coupon, class Fixed>
void host_chunk_walk(const scen::HostBatch& b, const int64_t* bounds, int64_t ch, const Coupon& coupon, const Fixed& fixed) {
    const scen::ChunkRange r = scen::host_chunk_range(ch, bounds, b.n);
    for (int64_t i = r.i0; i < r.i1; ++i) {
        const TradeRef tr{b.fix_off[i], b.flt_off[i], static_cast<int>(b.fix_off[i + 1] - b.fix_off[i]),
                          static_cast<int>(b.flt_off[i + 1] - b.flt_off[i]), b.notional[i], b.spread[i], b.fix_sign[i], b.flt_sign[i]};
        for (int c = 0; c < tr.n_flt; ++c) coupon(tr, i, c);
        for (int c = 0; c < tr.n_fix; ++c) fixed(tr, i, c);
    }
}

// LJ[k][p] on the host's tables (curve_tables.hpp's tiled layout).
inline double host_lj(const CurveTables& t, int k, int p) {
    return t.lj[(static_cast<size_t>(p / kPillarPad) * t.Kc + k) * kPillarPad + p % kPillarPad];
}

// o = [pv, delta[Q], gamma[Q][Q]] of one desk from its sums rec = [pv, w, D, O, ...]: zeros, then pv and the curve block
// delta[P], gamma[P][P] by project_curve_block's expression and order.
inline void host_project_curve(const CurveTables& t, const Request& rq, const double* rec, int Q, double* o) {
    const int P = t.P, Kc = t.Kc;
    const double *w = rec + 1, *D = w + Kc, *O = D + Kc;
    std::fill(o, o + 1 + Q + static_cast<size_t>(Q) * Q, 0.0);
    o[0] = rec[0];
    for (int q = 0; rq.delta && q < P; ++q) {
        double tot = 0.0;
        for (int wave = 0; wave < kProjWaves; ++wave) {
            double s = 0.0;
            for (int k = wave; k < Kc; k += kProjWaves) s = delta_step(s, w[k], host_lj(t, k, q));
            tot = wave == 0 ? s : tot + s;
        }
        o[1 + q] = tot * 1e-4;
    }
    for (int p = 0; rq.gamma && p < P; ++p)
        for (int q = 0; q < P; ++q) {
            double tot = 0.0;
            for (int wave = 0; wave < kProjWaves; ++wave) {
                double s = 0.0;
                for (int k = wave; k < Kc; k += kProjWaves) {
                    const bool next = k + 1 < Kc;
                    s = gamma_step(s, w[k], D[k], next ? O[k] : 0.0, host_lj(t, k, p), host_lj(t, k, q),
                                   next ? host_lj(t, k + 1, p) : 0.0, next ? host_lj(t, k + 1, q) : 0.0,
                                   t.lc[(static_cast<size_t>(k) * P + p) * P + q]);
                }
                tot = wave == 0 ? s : tot + s;
            }
            o[1 + Q + static_cast<size_t>(p) * Q + q] = tot * 1e-8;
        }
}

}  // namespace sbl
}  // namespace adr
