// What the sub-book ladder sources (subbook_ladder.hip, credit_subbook_ladder.hip) have in common, once: the folding of a
// trade's cash flows into knot-space nodes, a node's lookup and its numbers, the steps of the projection, the owner search
// of the knot kernels and the request and refusal wording.  These are what the host twins and the device are held to bit
// for bit, so a fix to any of them is made here.  The kernels and their entries stay in their sources.
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

// LJ[k][p] on the host's tables (curve_tables.hpp's tiled layout).
inline double host_lj(const CurveTables& t, int k, int p) {
    return t.lj[(static_cast<size_t>(p / kPillarPad) * t.Kc + k) * kPillarPad + p % kPillarPad];
}

}  // namespace sbl
}  // namespace adr
