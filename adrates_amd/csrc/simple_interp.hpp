// InterpolatorAd.simple_interpolate (cavour/market/curves/interpolator_ad.py:186-249, restated as
// oracle/cavour_oracle.py::simple_interpolate) on a raw knot table, for the host and the device alike.  Used by the
// YoY inflation kernel (yoy_risk.hip).  curve_lookup.hpp is the same rule on the uploaded curves' compacted tables;
// this header needs no tables: knots may repeat (the engine grid keeps duplicate times), the first of equal knots wins.
//
// The rule, for a query time t on knots x[0..K-1]:
//   - snap: the nearest knot (jnp.argmin: the first index on a tie) when it lies within 1e-10 of t -> that knot's value;
//   - otherwise evaluate at tau = t + 1e-12 with jnp.interp: segment i = clip(searchsorted(x, tau, 'right'), 1, K-1),
//     ordinate lo + w (hi - lo), w = (tau - x[i-1]) / dx, fp[i-1] where |dx| <= 2^-104, and fp[0] / fp[K-1] (constant)
//     below / above the knot range;
//   - ordinates: LINEAR_ZERO_RATES r_k = -ln(d_k) / max(x_k, 1e-15) (so r = 0 at a t = 0 knot with d = 1) and
//     D = exp(-r t); FLAT_FWD_RATES -ln(d_k) and D = exp(-f); LINEAR_FWD_RATES d_k itself.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/adrates.h"

namespace adr {
namespace si {

constexpr double kSnap = 1e-10;
constexpr double kShift = 1e-12;
constexpr double kTinyDx = 0x1p-104;        // np.spacing(np.finfo(float64).eps)

// Where t falls: ``snap`` >= 0 is the snapped knot; else ``lo`` / ``hi`` are the segment's knots and ``w`` the weight of
// ``hi`` (w = 0 and lo = hi for the dx guard and for the clamped ends).
struct Where {
    int snap, lo, hi;
    double w;
};

__host__ __device__ inline Where locate(double t, const double* x, int K) {
#pragma clang fp contract(off)
    int lo = 0, hi = K;                     // j = first knot later than t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int j = lo;
    double best_dist = INFINITY;
    int best = -1;
    if (j > 0) {
        best = j - 1;
        while (best > 0 && x[best - 1] == x[best]) --best;
        best_dist = fabs(t - x[best]);
    }
    if (j < K) {
        const double dh = fabs(t - x[j]);
        if (dh < best_dist) { best_dist = dh; best = j; }
    }
    Where r;
    if (best_dist < kSnap) {
        r.snap = best; r.lo = r.hi = best; r.w = 0.0;
        return r;
    }
    r.snap = -1;
    const double tau = t + kShift;
    if (tau < x[0]) { r.lo = r.hi = 0; r.w = 0.0; return r; }
    if (tau > x[K - 1]) { r.lo = r.hi = K - 1; r.w = 0.0; return r; }
    // no knot lies in (t, tau] (it would have snapped), so searchsorted(tau, 'right') == j
    const int i = j < 1 ? 1 : (j > K - 1 ? K - 1 : j);
    const double dx = x[i] - x[i - 1];
    r.lo = i - 1;
    if (fabs(dx) <= kTinyDx) { r.hi = i - 1; r.w = 0.0; return r; }
    r.hi = i;
    r.w = (tau - x[i - 1]) / dx;
    return r;
}

__host__ __device__ inline double ordinate(const double* x, const double* d, int k, int method) {
    if (method == ADR_INTERP_LINEAR_ZERO_RATES) return -log(d[k]) / fmax(x[k], 1e-15);
    if (method == ADR_INTERP_FLAT_FWD_RATES) return -log(d[k]);
    return d[k];
}

// The discount factor at t (the value simple_interpolate returns).
__host__ __device__ inline double df(double t, const double* x, const double* d, int K, int method) {
#pragma clang fp contract(off)
    const Where p = locate(t, x, K);
    if (p.snap >= 0) return d[p.snap];
    const double flo = ordinate(x, d, p.lo, method);
    double f = flo;
    if (p.hi != p.lo) f = flo + p.w * (ordinate(x, d, p.hi, method) - flo);
    if (method == ADR_INTERP_LINEAR_ZERO_RATES) return exp(-f * t);
    if (method == ADR_INTERP_FLAT_FWD_RATES) return exp(-f);
    return f;
}

// ln D(t) = w_a L_a + w_b L_b in weight form, for a table whose knot 0 is (0, 1) and whose ordinates are L_k = ln d_k
// (the inflation curve: ln I).  Only LINEAR_ZERO_RATES and FLAT_FWD_RATES, whose ln D is linear in the L_k.  Knot 0
// has L = 0; it is returned as index 0 and the caller drops it.  wb = 0 (and b = a) for a single knot.
struct LogWeights {
    int a, b;
    double wa, wb;
};

__host__ __device__ inline LogWeights log_weights(double t, const double* x, int K, int method) {
#pragma clang fp contract(off)
    const Where p = locate(t, x, K);
    LogWeights r;
    r.a = r.b = p.lo; r.wa = 1.0; r.wb = 0.0;
    if (p.snap >= 0) return r;                              // ln d at the knot
    const bool lz = method == ADR_INTERP_LINEAR_ZERO_RATES;
    if (p.hi == p.lo) {                                     // clamped end or dx guard: the knot's ordinate held
        if (lz) r.wa = t / fmax(x[p.lo], 1e-15);            // ln D = -r t = t L / x  (r_0 = 0: L_0 = 0)
        return r;
    }
    r.b = p.hi;
    if (lz) {
        r.wa = t * (1.0 - p.w) / fmax(x[p.lo], 1e-15);
        r.wb = t * p.w / x[p.hi];
    } else {
        r.wa = 1.0 - p.w;
        r.wb = p.w;
    }
    return r;
}

}  // namespace si
}  // namespace adr
