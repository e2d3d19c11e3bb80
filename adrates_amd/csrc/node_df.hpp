// Discount factors on a curve's OWN node set (market/curves/interpolator.py::_point), shared by the bond and FRN
// measures (bond_measures.hip, frn_measures.hip).  Not curve_lookup.hpp's engine interpolation, which snaps knots and
// treats the ends differently.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/adrates.h"

namespace adr {

// interpolator.py::_point: ``i`` is the first node with x[i] >= t (the reference's linear scan stops at n - 1), n when t
// lies beyond the last node.  A time before the first node has no formula there; it gives NaN.
__host__ __device__ inline double node_df(double t, const double* x, const double* d, int n, int method) {
#pragma clang fp contract(off)      // the host and device twins evaluate the same expressions, without fma
    if (t == x[0]) return d[0];
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (x[mid] < t) lo = mid + 1; else hi = mid;
    }
    int i = lo;
    if (t > x[i]) i = n;
    if (i == 0) return NAN;
    if (method == ADR_INTERP_LINEAR_ZERO_RATES) {
        double r1, r2, a, b;
        if (i == 1) {                       // first segment: the first node's zero rate held flat
            r1 = r2 = -log(d[1]) / x[1];
            a = x[0]; b = x[1];
        } else if (i < n) {
            r1 = -log(d[i - 1]) / x[i - 1];
            r2 = -log(d[i]) / x[i];
            a = x[i - 1]; b = x[i];
        } else {                            // extrapolation: the last node's zero rate held flat
            r1 = r2 = -log(d[n - 1]) / x[n - 1];
            a = x[n - 2]; b = x[n - 1];
        }
        const double rate = ((b - t) * r1 + (t - a) * r2) / (b - a);
        return exp(-rate * t);
    }
    if (method == ADR_INTERP_FLAT_FWD_RATES) {   // -ln(df) linear; the last segment's slope beyond the last node
        const int a = i < n ? i - 1 : n - 2, b = i < n ? i : n - 1;
        const double rt1 = -log(d[a]), rt2 = -log(d[b]);
        const double rt = ((x[b] - t) * rt1 + (t - x[a]) * rt2) / (x[b] - x[a]);
        return exp(-rt);
    }
    // LINEAR_FWD_RATES: forwards of the segments interpolated; `small` regularises the first segment as the reference does
    const double small = 1e-10;
    if (i == 1) return exp(-(t * -log(d[1] + small) / (x[1] + small)));
    const double fwd1 = -log(d[i - 1] / d[i - 2]) / (x[i - 1] - x[i - 2]);
    double fwd = fwd1;
    if (i < n) {
        const double fwd2 = -log(d[i] / d[i - 1]) / (x[i] - x[i - 1]);
        fwd = ((x[i] - t) * fwd1 + (t - x[i - 1]) * fwd2) / (x[i] - x[i - 1]);
    }
    return d[i - 1] * exp(-fwd * (t - x[i - 1]));
}

}  // namespace adr
