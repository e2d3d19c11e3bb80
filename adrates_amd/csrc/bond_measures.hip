// Batched spread and yield measures of fixed-rate bonds (adr_bond_measures*; declarations: include/adrates.h).
//
// Per bond, the host methods of adrates_amd/trades/credit/bond.py (cavour/trades/credit/bond.py:262-783):
//   1. z from the target dirty value when a clean price is given (`z_spread`),
//   2. the price at z and dv01 = cs01 from z -/+ 1bp (`value`, `dv01`, `cs01`),
//   3. the yield whose yield-PV equals that dirty value (`yield_to_maturity`),
//   4. Macaulay duration and convexity at that yield (`duration`, `convexity`).
// Discount factors come from the curve's OWN node set, interpolated like market/curves/interpolator.py::_point
// (not curve_lookup.hpp's engine interpolation, which snaps knots and treats the ends differently).
//
// Layout (measures_common.hpp): kGroup lanes per bond; the first kRegFlows flows of each lane stay in VGPRs across the
// solver's iterations, later ones (long bonds) are re-derived from global memory on every pass.  The host entry point runs
// the same per-bond code with the same per-lane order and the same reduction tree.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "host_pool.hpp"
#include "measures_common.hpp"
#include "node_df.hpp"

// The host and the device evaluate the same expressions; no contraction into fma, so the two differ only by their
// exp / log implementations.
#pragma clang fp contract(off)

namespace adr {
namespace bond {

using namespace meas;

constexpr int kRegFlows = 8;                // flows per lane held in registers (kGroup * kRegFlows = 128 per bond)
static_assert(ADR_BOND_MAX_NODES == kMaxNodes, "measures_common.hpp's checks");

enum Kind { Z_NEWTON = 0, Z_PRICES = 1, Y_NEWTON = 2, Y_MOMENTS = 3 };

struct Args {
    int method, n_nodes;
    const double* node_t;
    const double* node_df;
    int64_t n;
    const int64_t* flow_off;
    const double* flow_T;
    const double* flow_tau;
    const double* flow_cpn;
    const double* flow_prin;
    const double* bond_Ts;
    const double* bond_tauM;
    const double* bond_face;
    const double* bond_acc100;
    const double* bond_quote;
    int quote_is_z;
    double* out;                            // [ADR_BOND_OUTPUTS][n]
    int32_t* status;
};

// What one flow adds to a pass.  A = (coupon + principal if > 0) * D(T) / D(T_s) is the flow on the curve (`value`
// discounts relative to the settlement date); c is the coupon alone (the yield measures price coupons plus the FULL face at
// the unadjusted maturity, whatever the amortization).
__host__ __device__ inline V3 term(int kind, double x, double A, double tau, double c) {
    switch (kind) {
    case Z_NEWTON: {
        const double e = A * exp(-x * tau);
        return {e, -(e * tau), 0.0};
    }
    case Z_PRICES:
        return {A * exp(-x * tau), A * exp(-(x - kBump) * tau), A * exp(-(x + kBump) * tau)};
    case Y_NEWTON: {
        const double e = c * exp(-x * tau);
        return {e, -(e * tau), 0.0};
    }
    default: {
        const double e = c * exp(-x * tau);
        return {e, e * tau, e * (tau * tau)};
    }
    }
}

// The face at the unadjusted maturity, added after the pass (bond.py:488-503, 648-750); tau_M <= 0: matured.
template <class Group>
__host__ __device__ inline V3 pass(Group& g, int kind, double x, double face, double tauM) {
    V3 s = g.sum(kind, x);
    if (kind >= Y_NEWTON && tauM > 0.0) {
        const V3 p = term(kind, x, 0.0, tauM, face);
        s = add(s, p);
    }
    return s;
}

using Result = meas::Result<ADR_BOND_OUTPUTS>;

template <class Group>
__host__ __device__ inline Result measures(Group& g, double face, double tauM, double acc100, double quote, int quote_is_z) {
    Result r;
    double z = quote;
    int sz = 0;
    if (!quote_is_z) {
        const double target = ((quote + acc100) / 100.0) * face;
        sz = solve([&](double x) { return pass(g, Z_NEWTON, x, face, tauM); }, target, -0.1, 0.5, 0.01, &z);
    }
    if (sz == 2) {                                          // nan_result(2), written in place: see the kernel
        for (int k = 0; k < ADR_BOND_OUTPUTS; ++k) r.v[k] = NAN;
        r.status = 2;
        return r;
    }
    const V3 p = pass(g, Z_PRICES, z, face, tauM);
    const double dirty = (p.a / face) * 100.0;
    const double clean = dirty - acc100;
    r.v[ADR_BOND_Z] = z;
    r.v[ADR_BOND_DIRTY] = dirty;
    r.v[ADR_BOND_CLEAN] = clean;
    r.v[ADR_BOND_DV01] = (p.b - p.c) / 2.0;
    double y = NAN;
    const int sy = solve([&](double x) { return pass(g, Y_NEWTON, x, face, tauM); }, ((clean + acc100) / 100.0) * face, -0.5, 0.5,
                         0.05, &y);
    r.v[ADR_BOND_YTM] = y;
    r.v[ADR_BOND_DURATION] = r.v[ADR_BOND_CONVEXITY] = NAN;
    if (sy != 2) {
        const V3 m = pass(g, Y_MOMENTS, y, face, tauM);
        r.v[ADR_BOND_DURATION] = m.b / m.a;
        r.v[ADR_BOND_CONVEXITY] = m.c / m.a;
    }
    r.status = sz > sy ? sz : sy;
    return r;
}

// ------------------------------------------------------------------------------------------------------------ device
struct DeviceGroup {
    const Args* a;
    const double* st;
    const double* sd;
    int lane;
    int64_t f0;
    int nf;
    double Ds;
    double A[kRegFlows], tau[kRegFlows], c[kRegFlows];

    __device__ void flow(int64_t i, double& Ai, double& ti, double& ci) const {
        const double T = a->flow_T[i], p = a->flow_prin[i];
        ci = a->flow_cpn[i];
        ti = a->flow_tau[i];
        Ai = (ci + (p > 0.0 ? p : 0.0)) * (node_df(T, st, sd, a->n_nodes, a->method) / Ds);
    }

    __device__ void load() {
#pragma unroll
        for (int k = 0; k < kRegFlows; ++k) {
            const int i = lane + k * kGroup;
            A[k] = tau[k] = c[k] = 0.0;
            if (i < nf) flow(f0 + i, A[k], tau[k], c[k]);
        }
    }

    __device__ V3 sum(int kind, double x) const {
        V3 s = {0.0, 0.0, 0.0};
#pragma unroll
        for (int k = 0; k < kRegFlows; ++k)
            if (lane + k * kGroup < nf) s = add(s, term(kind, x, A[k], tau[k], c[k]));
        for (int i = lane + kRegFlows * kGroup; i < nf; i += kGroup) {
            double Ai, ti, ci;
            flow(f0 + i, Ai, ti, ci);
            s = add(s, term(kind, x, Ai, ti, ci));
        }
        return group_sum(s);
    }
};

__global__ __launch_bounds__(kBlock) void bond_measures_kernel(Args a) {
    __shared__ double s_t[ADR_BOND_MAX_NODES], s_d[ADR_BOND_MAX_NODES];
    for (int k = threadIdx.x; k < a.n_nodes; k += kBlock) {
        s_t[k] = a.node_t[k];
        s_d[k] = a.node_df[k];
    }
    __syncthreads();
    const int64_t b = static_cast<int64_t>(blockIdx.x) * kPerBlock + threadIdx.x / kGroup;
    if (b >= a.n) return;
    const int lane = threadIdx.x % kGroup;
    const int64_t f0 = a.flow_off[b], f1 = a.flow_off[b + 1];
    Result r;
    // malformed offsets: no reads, NaN and status 2 - nan_result(2), written in place here and in measures because the
    // call orders the constant moves of these paths differently, and the kernel's instructions are kept as they were
    if (f1 < f0 || f1 - f0 > kMaxFlows) {
        for (int k = 0; k < ADR_BOND_OUTPUTS; ++k) r.v[k] = NAN;
        r.status = 2;
    } else {
        DeviceGroup g;
        g.a = &a; g.st = s_t; g.sd = s_d; g.lane = lane; g.f0 = f0; g.nf = static_cast<int>(f1 - f0);
        g.Ds = node_df(a.bond_Ts[b], s_t, s_d, a.n_nodes, a.method);
        g.load();
        r = measures(g, a.bond_face[b], a.bond_tauM[b], a.bond_acc100[b], a.bond_quote[b], a.quote_is_z);
    }
    // lanes 0 .. 6 store one output each, lane 7 the status
    for (int k = 0; k < ADR_BOND_OUTPUTS; ++k)
        if (lane == k) a.out[static_cast<int64_t>(k) * a.n + b] = r.v[k];
    if (lane == ADR_BOND_OUTPUTS) a.status[b] = r.status;
}

// -------------------------------------------------------------------------------------------------------------- host
struct HostGroup {
    const double* A;
    const double* tau;
    const double* c;
    int nf;

    V3 sum(int kind, double x) const {
        return host_group_sum(nf, [&](int i) { return term(kind, x, A[i], tau[i], c[i]); });
    }
};

int validate(const char* who, int method, int n_nodes, const double* node_t, const double* node_df, int64_t n,
             const void* off, const void* T, const void* tau, const void* cpn, const void* prin, const void* Ts,
             const void* tauM, const void* face, const void* acc, const void* quote, const void* out, const void* status) {
    const std::string w(who);
    int rc = check_scheme(w, method);
    if (rc == ADR_OK) rc = check_node_table(w, n_nodes, node_t, node_df, ": the curve needs 2 .. ADR_BOND_MAX_NODES (1024) nodes");
    if (rc != ADR_OK) return rc;
    if (n < 0 || (n > 0 && (!off || !Ts || !tauM || !face || !acc || !quote || !out || !status)))
        return adr_set_error(ADR_ERR_INVALID, w + ": bad count / null array");
    (void)T; (void)tau; (void)cpn; (void)prin;
    return ADR_OK;
}

int check_host_arrays(const char* who, int n_nodes, const double* node_t, int64_t n, const int64_t* off, const double* T,
                      const double* tau, const double* cpn, const double* prin, const double* Ts) {
    const std::string w(who);
    int rc = check_node_times(w, n_nodes, node_t);
    if (rc != ADR_OK || n == 0) return rc;
    if (off[0] != 0) return adr_set_error(ADR_ERR_INVALID, w + ": flow_off[0] must be 0");
    rc = check_offsets(w, n, off, "flow");
    if (rc != ADR_OK) return rc;
    const int64_t m = off[n];
    if (m > 0 && (!T || !tau || !cpn || !prin)) return adr_set_error(ADR_ERR_INVALID, w + ": null flow arrays");
    for (int64_t i = 0; i < m; ++i)
        if (!(T[i] >= node_t[0]) || !std::isfinite(T[i]) || !std::isfinite(tau[i]) || !std::isfinite(cpn[i]) ||
            !std::isfinite(prin[i]))
            return adr_set_error(ADR_ERR_INVALID, w + ": flow times must be finite and not before the curve's first node");
    for (int64_t b = 0; b < n; ++b)
        if (!(Ts[b] >= node_t[0]) || !std::isfinite(Ts[b]))
            return adr_set_error(ADR_ERR_INVALID, w + ": settlement times must be finite and not before the curve's first node");
    return ADR_OK;
}

}  // namespace bond
}  // namespace adr

namespace B = adr::bond;

extern "C" {

int adr_bond_measures_dev(adr_ctx* ctx, int interp_method, int n_nodes, const double* node_t, const double* node_df, int64_t n,
                          const int64_t* flow_off, const double* flow_T, const double* flow_tau, const double* flow_cpn,
                          const double* flow_prin, const double* bond_Ts, const double* bond_tauM, const double* bond_face,
                          const double* bond_acc100, const double* bond_quote, int quote_is_z, double* out, int32_t* status,
                          void* stream_v) {
    int rc = B::validate("adr_bond_measures_dev", interp_method, n_nodes, node_t, node_df, n, flow_off, flow_T, flow_tau,
                         flow_cpn, flow_prin, bond_Ts, bond_tauM, bond_face, bond_acc100, bond_quote, out, status);
    if (rc != ADR_OK) return rc;
    const B::Args a{interp_method, n_nodes, node_t, node_df, n, flow_off, flow_T, flow_tau, flow_cpn, flow_prin, bond_Ts, bond_tauM,
                    bond_face, bond_acc100, bond_quote, quote_is_z ? 1 : 0, out, status};
    return adr::meas::launch("adr_bond_measures_dev", ctx, stream_v, B::bond_measures_kernel, a, "bonds");
}

int adr_bond_measures(adr_ctx* ctx, int interp_method, int n_nodes, const double* node_t, const double* node_df, int64_t n,
                      const int64_t* flow_off, const double* flow_T, const double* flow_tau, const double* flow_cpn,
                      const double* flow_prin, const double* bond_Ts, const double* bond_tauM, const double* bond_face,
                      const double* bond_acc100, const double* bond_quote, int quote_is_z, double* out, int32_t* status) {
    const char* who = "adr_bond_measures";
    int rc = B::validate(who, interp_method, n_nodes, node_t, node_df, n, flow_off, flow_T, flow_tau, flow_cpn, flow_prin,
                         bond_Ts, bond_tauM, bond_face, bond_acc100, bond_quote, out, status);
    if (rc == ADR_OK) rc = B::check_host_arrays(who, n_nodes, node_t, n, flow_off, flow_T, flow_tau, flow_cpn, flow_prin, bond_Ts);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::meas::target_stream(who, ctx, n, nullptr, &stream);
    if (rc != ADR_OK || n == 0) return rc;
    const int64_t m = flow_off[n];
    double *dt, *dd, *dT, *dtau, *dcpn, *dprin, *dTs, *dtauM, *dface, *dacc, *dquote, *dout;
    int64_t* doff;
    int32_t* dstatus;
    adr::call::Staging mem;
    mem.in(&dt, node_t, n_nodes);
    mem.in(&dd, node_df, n_nodes);
    mem.in(&dT, flow_T, m);
    mem.in(&dtau, flow_tau, m);
    mem.in(&dcpn, flow_cpn, m);
    mem.in(&dprin, flow_prin, m);
    mem.in(&dTs, bond_Ts, n);
    mem.in(&dtauM, bond_tauM, n);
    mem.in(&dface, bond_face, n);
    mem.in(&dacc, bond_acc100, n);
    mem.in(&dquote, bond_quote, n);
    mem.in(&doff, flow_off, n + 1);
    mem.out(&dout, out, ADR_BOND_OUTPUTS * static_cast<size_t>(n));
    mem.out(&dstatus, status, n);
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess)
        rc = adr_bond_measures_dev(ctx, interp_method, n_nodes, dt, dd, n, doff, dT, dtau, dcpn, dprin, dTs, dtauM, dface, dacc,
                                   dquote, quote_is_z, dout, dstatus, stream);
    return mem.finish(who, rc, e, stream);
}

int adr_bond_measures_host(int interp_method, int n_nodes, const double* node_t, const double* node_df, int64_t n,
                           const int64_t* flow_off, const double* flow_T, const double* flow_tau, const double* flow_cpn,
                           const double* flow_prin, const double* bond_Ts, const double* bond_tauM, const double* bond_face,
                           const double* bond_acc100, const double* bond_quote, int quote_is_z, double* out, int32_t* status) {
    const char* who = "adr_bond_measures_host";
    int rc = B::validate(who, interp_method, n_nodes, node_t, node_df, n, flow_off, flow_T, flow_tau, flow_cpn, flow_prin,
                         bond_Ts, bond_tauM, bond_face, bond_acc100, bond_quote, out, status);
    if (rc == ADR_OK) rc = B::check_host_arrays(who, n_nodes, node_t, n, flow_off, flow_T, flow_tau, flow_cpn, flow_prin, bond_Ts);
    if (rc != ADR_OK || n == 0) return rc;
    adr::parallel_ranges(n, adr::pool_threads(n, 256), [&](int, int64_t lo, int64_t hi) {
        std::vector<double> A;
        for (int64_t b = lo; b < hi; ++b) {
            const int64_t f0 = flow_off[b];
            const int nf = static_cast<int>(flow_off[b + 1] - f0);
            const double Ds = adr::node_df(bond_Ts[b], node_t, node_df, n_nodes, interp_method);
            A.resize(static_cast<size_t>(nf));
            for (int i = 0; i < nf; ++i) {
                const double p = flow_prin[f0 + i];
                A[i] = (flow_cpn[f0 + i] + (p > 0.0 ? p : 0.0)) *
                       (adr::node_df(flow_T[f0 + i], node_t, node_df, n_nodes, interp_method) / Ds);
            }
            B::HostGroup g{A.data(), flow_tau + f0, flow_cpn + f0, nf};
            const B::Result r = B::measures(g, bond_face[b], bond_tauM[b], bond_acc100[b], bond_quote[b], quote_is_z ? 1 : 0);
            for (int k = 0; k < ADR_BOND_OUTPUTS; ++k) out[static_cast<int64_t>(k) * n + b] = r.v[k];
            status[b] = r.status;
        }
    });
    return ADR_OK;
}

}  // extern "C"
