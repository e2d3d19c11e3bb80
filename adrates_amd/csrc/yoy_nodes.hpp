// A YoY coupon on the inflation curve's nodes, once: the nodes L_k = T_k ln(1 + b_k) with their derivatives, the coupon's
// at most four live slots with u = c L' and v = c L'', its projected amount, and the (p, q) entry of its gamma update.
// Shared by yoy_risk.hip (per-swap and book Greeks) and yoy_subbook_ladder.hip (per-desk ladders); the formulas are derived
// at the top of yoy_risk.hip, from which this code was moved unchanged.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/adrates.h"
#include "simple_interp.hpp"

#pragma clang fp contract(off)      // the host and the device evaluate the same expressions

namespace adr {
namespace yoy {

constexpr int kNodes = ADR_YOY_MAX_PILLARS + 1;

// The unit discount grid under ADR_INTERP_LINEAR_FWD_RATES: si::df returns 1.0 exactly for every date.
constexpr double kUnitX[2] = {0.0, 1.0}, kUnitD[2] = {1.0, 1.0};

// The inflation curve's nodes: x[0] = 0 with L = L' = L'' = 0, then the pillars.
struct Infl {
    const double *x, *L, *L1, *L2;
    int n, method;
};

__host__ __device__ inline void make_node(const double* T, const double* b, int k, double* x, double* L, double* L1,
                                          double* L2) {
    if (k == 0) { *x = 0.0; *L = 0.0; *L1 = 0.0; *L2 = 0.0; return; }
    const double t = T[k - 1], ob = 1.0 + b[k - 1];
    *x = t;
    *L = t * log(ob);
    *L1 = t / ob;
    *L2 = -(t / (ob * ob));
}

// One coupon: its projected amount, its PV and its inflation-curve terms.  k[j] = pillar index + 1 (knot index), or -1.
// g = scale D(tp) / D0 (1 + y), 0 like pv for a coupon that is not live.  On the unit grid kUnitX / kUnitD (D = 1 at every
// date, no exp or log on the way) and D0 = 1.0 they are scale (1 + y) and the amount under the mask: what a caller with a
// discount factor of its own multiplies by it (yoy_subbook_ladder.hip).
struct Desc {
    int k[4];
    double u[4], v[4];
    double g, pv, amount;
};

__host__ __device__ inline Desc describe(const double* dx, const double* dd, int K, int dm, double D0, const Infl& f,
                                         const double* cpn, int64_t m, int64_t i) {
    const double tp = cpn[ADR_YOY_TP * m + i], ts = cpn[ADR_YOY_TS * m + i], te = cpn[ADR_YOY_TE * m + i];
    const double scale = cpn[ADR_YOY_SCALE * m + i], spread = cpn[ADR_YOY_SPREAD * m + i];
    const si::LogWeights we = si::log_weights(te, f.x, f.n, f.method), ws = si::log_weights(ts, f.x, f.n, f.method);
    Desc d;
    double c[4] = {we.wa, we.wb, -ws.wa, -ws.wb};
    d.k[0] = we.a; d.k[1] = we.b; d.k[2] = ws.a; d.k[3] = ws.b;
    // merge repeated knots into their first slot; drop knot 0 and zero coefficients
    for (int j = 0; j < 4; ++j) {
        if (d.k[j] == 0) { d.k[j] = -1; continue; }
        for (int q = 0; q < j; ++q)
            if (d.k[q] == d.k[j]) { c[q] = c[q] + c[j]; d.k[j] = -1; break; }
    }
    double lnr = 0.0;
    for (int j = 0; j < 4; ++j) {
        if (d.k[j] > 0 && c[j] == 0.0) d.k[j] = -1;
        if (d.k[j] > 0) lnr = lnr + c[j] * f.L[d.k[j]];
    }
    const double one_y = exp(lnr);
    d.amount = scale * ((one_y - 1.0) + spread);
    const bool live = tp > 0.0;                                 // the engine's strict tp > value time mask
    const double dfr = si::df(tp, dx, dd, K, dm) / D0;
    d.pv = live ? d.amount * dfr : 0.0;
    d.g = live ? (scale * dfr) * one_y : 0.0;
    for (int j = 0; j < 4; ++j) {
        d.u[j] = d.k[j] > 0 ? c[j] * f.L1[d.k[j]] : 0.0;
        d.v[j] = d.k[j] > 0 ? c[j] * f.L2[d.k[j]] : 0.0;
    }
    return d;
}

// The (p, q) entry of a coupon's gamma update (p, q: slots 0-3).
__host__ __device__ inline double gamma_term(double up, double uq, double vp, bool diag) {
    double val = up * uq;
    if (diag) val = val + vp;
    return val;
}

}  // namespace yoy
}  // namespace adr
