// What the measures sources (bond_measures.hip, frn_measures.hip) have in common, once: the lane group and its fixed
// summation order, the root finder, the result record, the host checks and the launch.  These are what the host twins
// and the device are held to bit for bit, so a fix to any of them is made here.  The flows, the per-instrument formulas
// and the kernels stay in their sources - also the kernels' two short loops that stage a node table and store a result:
// as functions of this header they compile to other register assignments than the loops written in the kernel.
//
// Layout they share: kGroup lanes per instrument, its flows dealt across the lanes (flow i on lane i % kGroup); a lane
// adds its flows in order, then one fixed-order butterfly over the group's lanes ends each pass, so every lane holds the
// same bits and an instrument's results do not depend on the launch shape.  The host runs the lanes in sequence and
// then the same tree.  The node tables are staged in LDS once per block.  No atomics.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/adrates.h"
#include "blocking_call.hpp"

// The host and the device evaluate the same expressions; no contraction into fma, so the two differ only by their
// exp / log implementations.  As in scenario_common.hpp, the pragma stands before the first expression of this header
// and stays in force to the end of the including source, which states it again for its own code.
#pragma clang fp contract(off)

namespace adr {
namespace meas {

constexpr int kGroup = 16;                  // lanes per instrument
constexpr int kBlock = 256;
constexpr int kPerBlock = kBlock / kGroup;  // instruments per block
constexpr int kMaxIter = 100;
constexpr double kBump = 0.0001;            // 1bp
constexpr int kMaxNodes = 1024;             // ADR_BOND_MAX_NODES, ADR_FRN_MAX_NODES
constexpr int64_t kMaxFlows = int64_t(1) << 30;     // per instrument

struct V3 {
    double a, b, c;
};

__host__ __device__ inline bool finite(double x) { return x - x == 0.0; }    // false for NaN and +-inf

__host__ __device__ inline V3 add(V3 p, V3 q) { return {p.a + q.a, p.b + q.b, p.c + q.c}; }

// Root of pass(x).a - target, pass(x).b its derivative.  The bracket [lo, hi] first (brentq's test: no sign change ->
// fall back); inside it a safeguarded Newton whose steps are clipped into the shrinking sign-change bracket (bisection
// when a step leaves it).  Without a bracket an unbracketed Newton from x0.  Stop when |step| <= 1e-15 max(1, |x|) or
// after kMaxIter steps.  Returns 0 (bracketed), 1 (fallback converged) or 2 (no root).
template <class Pass>
__host__ __device__ inline int solve(Pass pass, double target, double lo, double hi, double x0, double* root) {
    V3 pa = pass(lo), pb = pass(hi);
    double fa = pa.a - target, fb = pb.a - target;
    if (fa == 0.0) { *root = lo; return 0; }
    if (fb == 0.0) { *root = hi; return 0; }
    if (fa * fb < 0.0) {
        double a = lo, b = hi;
        double x = a - fa / pa.b;
        if (!(x > a && x < b)) x = 0.5 * (a + b);
        for (int it = 0; it < kMaxIter; ++it) {
            const V3 p = pass(x);
            const double f = p.a - target;
            if (f == 0.0) break;
            if ((f < 0.0) == (fa < 0.0)) { a = x; fa = f; } else { b = x; }
            double xn = x - f / p.b;
            if (!(xn > fmin(a, b) && xn < fmax(a, b))) xn = 0.5 * (a + b);
            const double step = xn - x;
            x = xn;
            if (fabs(step) <= 1e-15 * fmax(1.0, fabs(x))) break;
        }
        *root = x;
        return 0;
    }
    double x = x0;
    for (int it = 0; it < kMaxIter; ++it) {
        const V3 p = pass(x);
        const double f = p.a - target;
        if (!finite(f) || !finite(p.b)) break;
        if (f == 0.0) { *root = x; return 1; }
        if (p.b == 0.0) break;
        const double xn = x - f / p.b;
        if (!finite(xn)) break;
        const double step = xn - x;
        x = xn;
        if (fabs(step) <= 1e-15 * fmax(1.0, fabs(x))) { *root = x; return 1; }
    }
    *root = NAN;
    return 2;
}

template <int kOutputs>
struct Result {
    double v[kOutputs];
    int32_t status;
};

template <int kOutputs>
__host__ __device__ inline Result<kOutputs> nan_result(int32_t status) {
    Result<kOutputs> r;
    for (int k = 0; k < kOutputs; ++k) r.v[k] = NAN;
    r.status = status;
    return r;
}

// ------------------------------------------------------------------------------------------------------------ device
// The end of a pass: the sum of the lanes' partial sums, the same bits on every lane of the group.
__device__ inline V3 group_sum(V3 s) {
#pragma unroll
    for (int m = kGroup / 2; m >= 1; m >>= 1) {
        s.a = s.a + __shfl_xor(s.a, m);
        s.b = s.b + __shfl_xor(s.b, m);
        s.c = s.c + __shfl_xor(s.c, m);
    }
    return s;
}

__device__ inline int group_or(int v) {
#pragma unroll
    for (int m = kGroup / 2; m >= 1; m >>= 1) v |= __shfl_xor(v, m);
    return v;
}

// -------------------------------------------------------------------------------------------------------------- host
// The device's lanes in sequence: lane l sums term(l), term(l + kGroup), ... in order, then the butterfly's tree (lane
// 0's view).
template <class Term>
inline V3 host_group_sum(int n, Term term) {
    V3 p[kGroup];
    for (int l = 0; l < kGroup; ++l) {
        p[l] = {0.0, 0.0, 0.0};
        for (int i = l; i < n; i += kGroup) p[l] = add(p[l], term(i));
    }
    for (int m = kGroup / 2; m >= 1; m >>= 1)
        for (int l = 0; l < m; ++l) p[l] = add(p[l], p[l + m]);
    return p[0];
}

// The first failing check decides an entry's message, so each entry calls these in its own order.
inline int check_scheme(const std::string& w, int method) {
    if (method != ADR_INTERP_FLAT_FWD_RATES && method != ADR_INTERP_LINEAR_FWD_RATES && method != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": only FLAT_FWD_RATES (1), LINEAR_FWD_RATES (2) and LINEAR_ZERO_RATES (4)");
    return ADR_OK;
}

// `needs` is the entry's own sentence about the node count.
inline int check_node_table(const std::string& w, int n_nodes, const double* t, const double* d, const char* needs) {
    if (n_nodes < 2 || n_nodes > kMaxNodes) return adr_set_error(ADR_ERR_UNSUPPORTED, w + needs);
    if (!t || !d) return adr_set_error(ADR_ERR_INVALID, w + ": null node arrays");
    return ADR_OK;
}

inline int check_node_times(const std::string& w, int n_nodes, const double* t) {
    for (int k = 0; k < n_nodes; ++k)
        if (!std::isfinite(t[k]) || (k > 0 && !(t[k] > t[k - 1])))
            return adr_set_error(ADR_ERR_INVALID, w + ": node times must be finite and increasing");
    return ADR_OK;
}

// `flows` is what the entry's message calls them.
inline int check_offsets(const std::string& w, int64_t n, const int64_t* off, const char* flows) {
    for (int64_t b = 0; b < n; ++b)
        if (off[b + 1] < off[b] || off[b + 1] - off[b] > kMaxFlows)
            return adr_set_error(ADR_ERR_INVALID, w + ": " + flows + " offsets must be non-decreasing");
    return ADR_OK;
}

// The stream of a call on n instruments (blocking_call.hpp's target_stream); an empty book ends the call after the
// check of the ctx, before the first HIP call.
inline int target_stream(const std::string& w, const adr_ctx* ctx, int64_t n, void* stream_or_null, hipStream_t* stream) {
    int device = 0;
    const int rc = adr_ctx_target(ctx, &device, stream);
    if (rc != ADR_OK || n == 0) return rc;
    return call::target_stream(w, ctx, static_cast<hipStream_t>(stream_or_null), stream);
}

// The tail of a _dev entry: the kernel on the call's stream, one group per instrument; `many` names the instruments.
template <class Kernel, class Args>
int launch(const std::string& w, const adr_ctx* ctx, void* stream_or_null, Kernel kernel, const Args& a, const char* many) {
    hipStream_t stream = nullptr;
    const int rc = target_stream(w, ctx, a.n, stream_or_null, &stream);
    if (rc != ADR_OK || a.n == 0) return rc;
    const int64_t blocks = (a.n + kPerBlock - 1) / kPerBlock;
    if (blocks > 0x7fffffff) return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": too many " + many + " for one launch");
    hipLaunchKernelGGL(kernel, dim3(static_cast<unsigned>(blocks)), dim3(kBlock), 0, stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

}  // namespace meas
}  // namespace adr
