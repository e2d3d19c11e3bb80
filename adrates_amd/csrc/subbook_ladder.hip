// Sub-book Greeks: per-desk PV, delta and gamma ladders of one batch on one curve from ONE launch chain
// (adr_subbook_ladders*; declarations and semantics: include/adrates.h).
//
// The book's ladder is a projection of its knot-space sums (kernels_knot.hip): per node omega = c exp(ba L[ka] + bb L[kb])
//     pv += omega,   w_k += omega b_k,   D_k += omega b_k^2,   O_ka += omega ba bb
// (under LINEAR_FWD_RATES a node is two single-knot amounts with weight 1 and no cross term).  Here those sums are kept per
// SUB-BOOK and projected once per sub-book:
//
//   1. subbook_knot_kernel: one wave takes one chunk of the sub-book plan (subbook.hpp: at most ADR_SCENARIO_CHUNK
//      consecutive trades, never across a sub-book boundary).  Lane l holds the header of the chunk's trade l; the chunk's
//      float coupons and fixed flows are two contiguous runs of the CSR arrays, walked 64 at a time, lane = flow.  A lane
//      finds its flow's trade with six steps over the lanes' headers, folds the coupon into nodes by the lite kernel's
//      rules (a coupon's start is the previous coupon's end: one node; a fixed flow paid with the coupon joins it), does
//      the lookup of each node's date (si::log_weights / si::locate, compact knots) and adds the node's numbers to the
//      wave's own tables in LDS.  A chunk starts from zeroed tables and ends by writing work[chunk] = [pv, w, D, O]: the
//      record depends on the chunk's trades alone.
//   2. sub::enqueue_sum adds every sub-book's records in the plan's order (chunk j to slot j % 64, then the halving tree).
//   3. subbook_project_kernel: out[b] = [pv, delta[P], gamma[P][P]], kernels_knot.hip's expression once per sub-book
//      (sbl::project_curve_block, subbook_ladder_common.hpp).
//
// Trades with ratio nodes (payment lag, per-coupon notionals) are refused.  The host twin (adr_subbook_ladders_host) runs
// the same node and projection code in the same chunks and summation orders on the CPU.  The projection, the knot launch,
// the checks of the handles and of the host arrays and the host's trade walk are subbook_ladder_common.hpp's, shared with
// credit_subbook_ladder.hip; this source keeps the knot kernel, its record and the order of each entry's checks.
#include "subbook_ladder_common.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace sbl {

// ------------------------------------------------------------------------------------------------------------ device
struct KnotArgs {
    CurveDev cv;
    TradesDev tr;
    int64_t chunk_cap;               // the rows `work` holds, an upper bound of the plan's count
    const int64_t *sub_chunks, *sub_bounds;      // the plan's chunk count and its [chunks][2] trade bounds (subbook.hpp)
    double* work;                    // [chunk_cap][S]
    int S, waves;
};

template <bool kLog, bool kGamma>
__device__ inline void add_node(const Amount& n, const double* s_x, const int16_t* s_comp, const double* s_log, int K, int Kc,
                                int method, double* tab, double& pv) {
    if (!n.on) return;
    const DateW d = lookup<kLog>(n.t, s_x, K, method, s_comp);
    const Terms t = node_terms<kLog>(d, n.a, s_log);
    const bool two = d.b != d.a;
    pv = pv + t.pv;
    // The bit contract rests on these LDS adds: where several lanes of ONE instruction add to the same address, the
    // hardware applies them in an order fixed by the lane ids and not by the table's base address, so a chunk's sums are
    // the same in whichever wave runs it.  gfx950 behaves so (tests: desk alone == desk in the book, run-to-run bits); it is
    // observed behaviour of ds_add_f64, not an architectural guarantee - a part or compiler that breaks it fails those tests.
    __hip_atomic_fetch_add(tab + d.a, t.wa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (two) __hip_atomic_fetch_add(tab + d.b, t.wb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (kGamma) {
        __hip_atomic_fetch_add(tab + Kc + d.a, t.da, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (two) {
            __hip_atomic_fetch_add(tab + Kc + d.b, t.db, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (kLog) __hip_atomic_fetch_add(tab + 2 * Kc + d.a, t.o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
}

template <bool kLog, bool kGamma>
__global__ __launch_bounds__(kWave * kMaxWaves) void subbook_knot_kernel(KnotArgs a) {
    constexpr int NT = kGamma ? 3 : 1;
    extern __shared__ double lds[];
    const int K = a.cv.K, Kc = a.cv.Kc, waves = a.waves;
    double* s_tab = lds;                                 // [waves][NT][Kc]
    double* s_x = s_tab + waves * NT * Kc;               // [K]
    double* s_log = s_x + K;                             // [Kc]
    int16_t* s_comp = reinterpret_cast<int16_t*>(s_log + Kc);      // [K]
    const int threads = kWave * waves;
    for (int i = threadIdx.x; i < waves * NT * Kc; i += threads) s_tab[i] = 0.0;
    for (int i = threadIdx.x; i < K; i += threads) {
        s_x[i] = a.cv.x[i];
        s_comp[i] = a.cv.compact_of[i];
    }
    for (int i = threadIdx.x; i < Kc; i += threads) s_log[i] = a.cv.log_df[i];
    __syncthreads();

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* tab = s_tab + wave * (NT * Kc);
    const Flows g{a.tr.fix_tp, a.tr.fix_pay, a.tr.flt_tp, a.tr.flt_ts, a.tr.flt_te, a.tr.flt_alpha};
    const int method = a.cv.method;
    int64_t n_chunks = *a.sub_chunks;                    // uniform: a scalar load
    n_chunks = n_chunks < a.chunk_cap ? n_chunks : a.chunk_cap;
    for (int64_t ch = static_cast<int64_t>(blockIdx.x) * waves + wave; ch < n_chunks; ch += static_cast<int64_t>(gridDim.x) * waves) {
        scen::ChunkRange r = scen::chunk_range<true>(ch, a.sub_bounds, a.tr.n);
        if (r.i1 > r.i0 + kChunk) r.i1 = r.i0 + kChunk;  // (a plan of build_plan never asks for more)
        const int cnt = r.i1 > r.i0 ? static_cast<int>(r.i1 - r.i0) : 0;
        TradeHeader h{};
        if (lane < cnt) h = a.tr.header[r.i0 + lane];
        double pv = 0.0;
        if (cnt > 0) {
            const int l_begin = scen::lane_int(h.flt_begin, 0), l_end = scen::lane_int(h.flt_begin + h.n_flt, cnt - 1);
            for (int base = l_begin; base < l_end; base += kWave) {
                const int f = base + lane;
                const TradeRef t = owner_trade(h, owner_lane(h.flt_begin, cnt, f));
                if (f < l_end) {
                    Amount pay, start;
                    float_nodes(g, t, static_cast<int>(f - t.l0), &pay, &start);
                    add_node<kLog, kGamma>(pay, s_x, s_comp, s_log, K, Kc, method, tab, pv);
                    add_node<kLog, kGamma>(start, s_x, s_comp, s_log, K, Kc, method, tab, pv);
                }
            }
            const int x_begin = scen::lane_int(h.fix_begin, 0), x_end = scen::lane_int(h.fix_begin + h.n_fix, cnt - 1);
            for (int base = x_begin; base < x_end; base += kWave) {
                const int f = base + lane;
                const TradeRef t = owner_trade(h, owner_lane(h.fix_begin, cnt, f));
                if (f < x_end) add_node<kLog, kGamma>(fixed_node(g, t, static_cast<int>(f - t.f0)), s_x, s_comp, s_log, K, Kc, method, tab, pv);
            }
        }
#pragma unroll
        for (int off = kWave / 2; off >= 1; off >>= 1) pv = pv + __shfl_xor(pv, off, kWave);
        wave_lds_order();
        double* rec = a.work + ch * a.S;
        if (lane == 0) rec[0] = pv;
        for (int k = lane; k < NT * Kc; k += kWave) {
            rec[1 + k] = tab[k];
            tab[k] = 0.0;
        }
        wave_lds_order();
    }
}

struct ProjectArgs {
    CurveDev cv;
    const double* sums;              // [B][S]
    int S;
    int64_t B;
    int want_delta, want_gamma;
    double* out;                     // [B][1 + P + P P]
};

__global__ __launch_bounds__(kWave * kProjWaves) void subbook_project_kernel(ProjectArgs a) { project_curve_block<false>(a); }

// -------------------------------------------------------------------------------------------------------------- host
inline int tables(bool gamma) { return gamma ? 3 : 1; }
inline int record_doubles(int Kc, bool gamma) { return 1 + tables(gamma) * Kc; }

// What an entry needs of its handles, checked.
int handles(const std::string& w, const adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, int64_t B, const Request& rq,
            Handles* h) {
    const int rc = check_handles(w, ctx, curve, trades, B, h);
    return rc != ADR_OK ? rc : check_fit(w, trades, *h, rq, tables(rq.gamma));
}

// The three steps on `stream`; every pointer is device memory.  work: adr_subbook_ladders_work doubles.
int enqueue(const std::string& w, adr_ctx* ctx, const Handles& h, int64_t B, const int64_t* plan, const Request& rq, double* out,
            double* work, hipStream_t stream_or_null) {
    if (!plan) return adr_set_error(ADR_ERR_INVALID, w + ": the sub-book plan is NULL (adr_scenario_subbook_plan fills it)");
    if (!out) return adr_set_error(ADR_ERR_INVALID, w + ": out is NULL");
    if (!work) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_subbook_ladders_work doubles are needed)");
    hipStream_t stream = nullptr;
    const int rc = call::target_stream(w, ctx, stream_or_null, &stream);
    if (rc != ADR_OK) return rc;
    const CurveDev& cv = *h.cv;
    const int S = record_doubles(cv.Kc, rq.gamma);
    const int64_t cap = sub::max_chunks(h.tr->n, B, kChunk);
    const sub::Plan pl = sub::plan_view(plan, B);
    double* sums = work + cap * S;                       // [B][S]
    const KnotGrid kg = knot_grid(ctx, cv, tables(rq.gamma), cap);
    const KnotArgs ka{cv, *h.tr, cap, pl.chunk_off + B, pl.bounds, work, S, kg.waves};
    const bool is_log = cv.method != ADR_INTERP_LINEAR_FWD_RATES;
    hipError_t e = launch_knot(rq.gamma ? (is_log ? &subbook_knot_kernel<true, true> : &subbook_knot_kernel<false, true>)
                                        : (is_log ? &subbook_knot_kernel<true, false> : &subbook_knot_kernel<false, false>),
                               ka, kg, stream);
    if (e == hipSuccess) e = sub::enqueue_sum(work, pl.chunk_off, cap, B, S, sums, stream);
    const int64_t tiles = (B + kProjDesks - 1) / kProjDesks;
    if (e == hipSuccess && tiles > INT32_MAX) e = hipErrorInvalidConfiguration;
    if (e == hipSuccess) {
        const ProjectArgs pa{cv, sums, S, B, rq.delta ? 1 : 0, rq.gamma ? 1 : 0, out};
        hipLaunchKernelGGL(subbook_project_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(cv.P + 1)),
                           dim3(kWave * kProjWaves), 0, stream, pa);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// The chunks [lo, hi) of the plan on the host: work[ch] = the chunk's record.
template <bool kLog>
void host_chunks(const CurveTables& t, int method, bool gamma, const scen::HostBatch& b, const int64_t* bounds, int S, double* work,
                 int64_t lo, int64_t hi) {
    const int K = t.K, Kc = t.Kc;
    const Flows g{b.fix_tp, b.fix_pay, b.flt_tp, b.flt_ts, b.flt_te, b.flt_alpha};
    for (int64_t ch = lo; ch < hi; ++ch) {
        double* rec = work + ch * S;
        std::fill(rec, rec + S, 0.0);
        auto add = [&](const Amount& n) {
            if (!n.on) return;
            const DateW d = lookup<kLog>(n.t, t.x.data(), K, method, t.compact_of.data());
            const Terms u = node_terms<kLog>(d, n.a, t.log_df.data());
            const bool two = d.b != d.a;
            rec[0] = rec[0] + u.pv;
            rec[1 + d.a] = rec[1 + d.a] + u.wa;
            if (two) rec[1 + d.b] = rec[1 + d.b] + u.wb;
            if (!gamma) return;
            rec[1 + Kc + d.a] = rec[1 + Kc + d.a] + u.da;
            if (two) {
                rec[1 + Kc + d.b] = rec[1 + Kc + d.b] + u.db;
                if (kLog) rec[1 + 2 * Kc + d.a] = rec[1 + 2 * Kc + d.a] + u.o;
            }
        };
        host_chunk_walk(
            b, bounds, ch,
            [&](const TradeRef& tr, int64_t, int c) {
                Amount pay, start;
                float_nodes(g, tr, c, &pay, &start);
                add(pay);
                add(start);
            },
            [&](const TradeRef& tr, int64_t, int c) { add(fixed_node(g, tr, c)); });
    }
}

// out[b] of the sub-books [lo, hi) from their sums: subbook_project_kernel's expression and order.
void host_project(const CurveTables& t, const Request& rq, const double* sums, int S, double* out, int64_t lo, int64_t hi) {
    const size_t stride = 1 + t.P + static_cast<size_t>(t.P) * t.P;
    for (int64_t b = lo; b < hi; ++b) host_project_curve(t, rq, sums + b * S, t.P, out + b * stride);
}

}  // namespace sbl
}  // namespace adr

namespace SL = adr::sbl;

extern "C" {

int adr_trades_ratio_flags_host(int64_t n, const int64_t* flt_off, const double* flt_tp, const double* flt_te,
                                const double* flt_alpha, const double* flt_weight, uint8_t* flags) {
    const std::string w = "adr_trades_ratio_flags_host";
    if (n < 0 || (n > 0 && (!flt_off || !flags))) return adr_set_error(ADR_ERR_INVALID, w + ": bad count / null array");
    if (n > 0 && flt_off[n] > 0 && (!flt_tp || !flt_te || !flt_alpha)) return adr_set_error(ADR_ERR_INVALID, w + ": null cash-flow array");
    adr::route::flag_lagged(0, n, flt_off, flt_tp, flt_te, flt_alpha, flt_weight, flags);
    return ADR_OK;
}

int64_t adr_subbook_ladders_work(const adr_curve* curve, int64_t n, int64_t B, uint32_t req_mask, int64_t* chunks) {
    const adr_ctx* owner = nullptr;
    const adr::CurveDev* cv = adr_curve_device_view(curve, &owner);
    if (!cv || n < 1 || B < 1) return 0;
    const int64_t cap = adr::sub::max_chunks(n, B, SL::kChunk);
    if (chunks) *chunks = cap;
    return (cap + B) * SL::record_doubles(cv->Kc, SL::request_of(req_mask).gamma);
}

int adr_subbook_ladders_dev(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, int64_t B, const int64_t* plan_dev,
                            uint32_t req_mask, double* out_dev, double* work_dev, void* stream) {
    const std::string w = "adr_subbook_ladders_dev";
    const SL::Request rq = SL::request_of(req_mask);
    SL::Handles h{};
    const int rc = SL::handles(w, ctx, curve, trades, B, rq, &h);
    if (rc != ADR_OK) return rc;
    return SL::enqueue(w, ctx, h, B, plan_dev, rq, out_dev, work_dev, static_cast<hipStream_t>(stream));
}

int adr_subbook_ladders(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, int64_t B, const int64_t* sub_off,
                        uint32_t req_mask, double* out) {
    const std::string w = "adr_subbook_ladders";
    const SL::Request rq = SL::request_of(req_mask);
    SL::Handles h{};
    int rc = SL::handles(w, ctx, curve, trades, B, rq, &h);
    if (rc != ADR_OK) return rc;
    if (!out) return adr_set_error(ADR_ERR_INVALID, w + ": out is NULL");
    std::vector<int64_t> plan;
    rc = adr::sub::build_plan(w, h.tr->n, B, sub_off, plan);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const int P = h.cv->P;
    double *dout, *dwork;
    int64_t* dplan;
    adr::call::Staging mem;                         // `plan` is uploaded from where it stands: it outlives finish()
    mem.out(&dout, out, static_cast<size_t>(B) * (1 + P + static_cast<size_t>(P) * P));
    mem.scratch(&dwork, static_cast<size_t>(adr_subbook_ladders_work(curve, h.tr->n, B, req_mask, nullptr)));
    mem.in(&dplan, plan.data(), plan.size());
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) rc = SL::enqueue(w, ctx, h, B, dplan, rq, dout, dwork, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_subbook_ladders_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac,
                             const double* hess, int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp,
                             const double* fix_pay, const double* flt_tp, const double* flt_ts, const double* flt_te,
                             const double* flt_alpha, const double* flt_weight, const double* notional, const double* spread,
                             const double* fix_sign, const double* flt_sign, int64_t B, const int64_t* sub_off, uint32_t req_mask,
                             double* out) {
    const std::string w = "adr_subbook_ladders_host";
    namespace SC = adr::scen;
    const SL::Request rq = SL::request_of(req_mask);
    const SL::HostCurve c{interp_method, K, P, times, dfs, jac, hess};
    const SC::HostBatch b{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional, spread,
                          fix_sign, flt_sign};
    int rc = SL::check_host_counts(w, interp_method, n, B);
    if (rc == ADR_OK) rc = SL::check_host_arrays(w, c, b, rq, out);
    if (rc == ADR_OK) rc = SL::check_host_trades(w, b);
    if (rc != ADR_OK) return rc;
    std::vector<int64_t> plan;
    rc = adr::sub::build_plan(w, n, B, sub_off, plan);
    if (rc != ADR_OK) return rc;
    adr::CurveTables t;
    rc = SL::host_tables(w, c, b, rq, t);
    if (rc != ADR_OK) return rc;
    const int S = SL::record_doubles(t.Kc, rq.gamma);
    const int64_t chunks = plan[B];
    std::vector<double> work(static_cast<size_t>(chunks) * S), sums(static_cast<size_t>(B) * S);
    const int64_t* bounds = plan.data() + B + 1;
    const bool lin = interp_method == ADR_INTERP_LINEAR_FWD_RATES;
    adr::parallel_ranges(chunks, adr::pool_threads(chunks, 4), [&](int, int64_t lo, int64_t hi) {
        if (lin) SL::host_chunks<false>(t, interp_method, rq.gamma, b, bounds, S, work.data(), lo, hi);
        else SL::host_chunks<true>(t, interp_method, rq.gamma, b, bounds, S, work.data(), lo, hi);
    });
    adr::sub::reduce_subbooks(work.data(), plan.data(), B, S, sums.data());
    adr::parallel_ranges(B, adr::pool_threads(B, 1), [&](int, int64_t lo, int64_t hi) {
        SL::host_project(t, rq, sums.data(), S, out, lo, hi);
    });
    return ADR_OK;
}

}  // extern "C"
