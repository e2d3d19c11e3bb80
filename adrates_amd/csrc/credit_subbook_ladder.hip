// Credit sub-book Greeks: per-desk PV, curve delta and gamma AT THE SPREADS, CS01 and spread gamma per credit bucket and
// the rate x spread cross gamma of one batch on one curve from ONE launch chain (adr_credit_subbook_ladders*;
// declarations and semantics: include/adrates.h).
//
// Trade i discounts every payment at D(tp) f, f = exp(-z_i tau), tau the flow's spread time (credit_scenario_pv.hip); the
// forward carries no spread.  Without ratio nodes a float coupon is N D(ts) f + N (s alpha - 1) D(tp) f and a fixed flow
// pay D(tp) f: the knot-space nodes of subbook_ladder.hip with their amounts scaled by f.  A node carries three amounts,
//     a = sum a_i f_i,   a1 = sum (-tau_i) a_i f_i,   a2 = sum tau_i^2 a_i f_i
// over the parts folded into it (each with its own tau), and with E the node's curve factor, evaluated once,
//     pv, w, D, O from a (subbook_ladder.hip),   cs += a1 E,   csg += a2 E,   wz_k += a1 E b_k.
// A trade has one bucket, so the spread-spread block is diagonal and the cross term of desk b and bucket g comes from the
// trades of that (desk, bucket) CELL alone.  The batch is ordered by (desk, bucket) and the chunk plan is cut over cells:
//
//   1. credit_subbook_knot_kernel: subbook_knot_kernel's structure - one wave per chunk of one cell, lane = flow, the owner
//      search over the lanes' headers, wavefront-scope LDS adds - with the trade's z in the lane, the spread times read
//      beside the flow and a fourth table wz per wave.  work[chunk] = [pv, w, D, O, wz, cs, csg] ([pv, w, cs] without GAMMA).
//   2. sub::enqueue_sum adds every cell's chunk records, then by the same rule every desk's cell sums.
//   3. credit_project_kernel writes the curve block of the augmented ladder out[b] = [pv, delta'[Q], gamma'[Q][Q]],
//      Q = P + G, from the desk sums (sbl::project_curve_block, the code subbook_project_kernel runs) and zeros elsewhere;
//      credit_cell_kernel then writes the spread rows and columns from the cell sums.
//
// Trades with ratio nodes are refused.  The host twin (adr_credit_subbook_ladders_host) runs the same node, sum and
// projection code in the same chunks and orders on the CPU.  The projection of the curve block, the knot launch, the
// checks of the handles and of the host arrays and the host's trade walk are subbook_ladder_common.hpp's, shared with
// subbook_ladder.hip; this source keeps the knot kernel, the cell kernel and the spread side's checks, which each entry
// puts between the shared ones in its own order.
#include "subbook_ladder_common.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace csl {

using namespace sbl;     // the shared pieces (subbook_ladder_common.hpp)

constexpr int kCellWaves = 4;       // cells per block of the cell kernel, one wave each

// ---------------------------------------------------------------------------------------------------- nodes (shared)
struct Taus {            // the spread times of a batch's flows
    const double *fix_tau, *flt_tau;
};

struct Amount3 {         // a node before its lookup: the amounts a, a1, a2 at time t
    double t, a, a1, a2;
    bool on;
};

// exp(-z tau); a trade without a spread has the factor 1.0 exactly, whatever tau holds.
__host__ __device__ inline double spread_factor(double z, double tau) { return z == 0.0 ? 1.0 : exp(-(z * tau)); }

// One part folded into a node: amount x at spread time tau.  The order of the products is stated here once.
__host__ __device__ inline void add_part(Amount3& n, double x, double z, double tau) {
    const double xf = x * spread_factor(z, tau);
    n.a = n.a + xf;
    n.a1 = n.a1 + (-tau) * xf;
    n.a2 = n.a2 + tau * (tau * xf);
}

__host__ __device__ inline bool live(const Amount3& n) { return n.a != 0.0 || n.a1 != 0.0 || n.a2 != 0.0; }

// sbl::float_nodes with the factors: the coupon's own amounts carry its f, the next coupon's start joins the payment node
// with the NEXT coupon's f, the fixed flow of the same index with its own.
__host__ __device__ inline void float_nodes(const Flows& g, const Taus& u, const TradeRef& r, double z, int c, Amount3* pay,
                                            Amount3* start) {
    const int64_t i = r.l0 + c;
    const double tp = g.flt_tp[i], ts = g.flt_ts[i], al = g.flt_alpha[i], tau = u.flt_tau[i];
    const bool valid = tp >= 0.0, accrues = al > 0.0;
    const double sn = r.flt_sign * r.notional;
    *pay = Amount3{tp, 0.0, 0.0, 0.0, false};
    add_part(*pay, valid ? sn * (r.spread * al - (accrues ? 1.0 : 0.0)) : 0.0, z, tau);
    if (c + 1 < r.n_flt && g.flt_alpha[i + 1] > 0.0 && g.flt_tp[i + 1] >= 0.0 && g.flt_ts[i + 1] == tp)
        add_part(*pay, sn, z, u.flt_tau[i + 1]);
    if (c < r.n_fix) {
        const double xt = g.fix_tp[r.f0 + c];
        if (xt == tp && xt > 0.0) add_part(*pay, r.fix_sign * g.fix_pay[r.f0 + c], z, u.fix_tau[r.f0 + c]);
    }
    pay->on = live(*pay);
    *start = Amount3{ts, 0.0, 0.0, 0.0, false};
    add_part(*start, sn, z, tau);
    start->on = valid && accrues && !(c > 0 && g.flt_tp[i - 1] == ts);
}

__host__ __device__ inline Amount3 fixed_node(const Flows& g, const Taus& u, const TradeRef& r, double z, int c) {
    const double xt = g.fix_tp[r.f0 + c];
    const bool merged = c < r.n_flt && g.flt_tp[r.l0 + c] == xt;
    Amount3 n{xt, 0.0, 0.0, 0.0, false};
    add_part(n, r.fix_sign * g.fix_pay[r.f0 + c], z, u.fix_tau[r.f0 + c]);
    n.on = !merged && xt > 0.0 && live(n);
    return n;
}

// The chunk record: [pv, w[Kc], D[Kc], O[Kc], wz[Kc], cs, csg], without GAMMA [pv, w[Kc], cs].
inline int tables(bool gamma) { return gamma ? 4 : 1; }
inline int record_doubles(int Kc, bool gamma) { return 1 + tables(gamma) * Kc + (gamma ? 2 : 1); }

// ------------------------------------------------------------------------------------------------------------ device
struct KnotArgs {
    CurveDev cv;
    TradesDev tr;
    const double* z;                 // [n]
    const int32_t* bucket;           // [n]
    Taus tau;
    int64_t n_fix, n_flt;            // the lengths of the spread-time arrays
    int G;
    int64_t chunk_cap;               // the rows `work` holds, an upper bound of the plan's count
    const int64_t *sub_chunks, *sub_bounds;      // the cell plan's chunk count and its [chunks][2] trade bounds (subbook.hpp)
    double* work;                    // [chunk_cap][S]
    int S, waves;
};

struct Sums {            // a lane's running sums
    double pv, cs, csg;
};

template <bool kLog, bool kGamma>
__device__ inline void add_node(const Amount3& n, const double* s_x, const int16_t* s_comp, const double* s_log, int K, int Kc,
                                int method, double* tab, Sums& s) {
    if (!n.on) return;
    const DateW d = lookup<kLog>(n.t, s_x, K, method, s_comp);
    const Factor e = node_factor<kLog>(d, s_log);
    const Terms t = node_terms_at<kLog>(d, n.a, e), t1 = node_terms_at<kLog>(d, n.a1, e);
    const bool two = d.b != d.a;
    s.pv = s.pv + t.pv;
    s.cs = s.cs + t1.pv;
    // As subbook_ladder.hip: the bit contract rests on the order in which the hardware applies the adds of ONE instruction
    // to the same address, which is fixed by the lane ids - observed behaviour of ds_add_f64 on gfx950, not a guarantee.
    __hip_atomic_fetch_add(tab + d.a, t.wa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (two) __hip_atomic_fetch_add(tab + d.b, t.wb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    if (kGamma) {
        s.csg = s.csg + node_terms_at<kLog>(d, n.a2, e).pv;
        __hip_atomic_fetch_add(tab + Kc + d.a, t.da, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (two) {
            __hip_atomic_fetch_add(tab + Kc + d.b, t.db, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
            if (kLog) __hip_atomic_fetch_add(tab + 2 * Kc + d.a, t.o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
        __hip_atomic_fetch_add(tab + 3 * Kc + d.a, t1.wa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        if (two) __hip_atomic_fetch_add(tab + 3 * Kc + d.b, t1.wb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
}

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, kWave);
    return v;
}

template <bool kLog, bool kGamma>
__global__ __launch_bounds__(kWave * kMaxWaves) void credit_subbook_knot_kernel(KnotArgs a) {
    constexpr int NT = kGamma ? 4 : 1;
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
        double z = 0.0;
        bool mine_ok = true;
        if (lane < cnt) {
            h = a.tr.header[r.i0 + lane];
            z = a.z[r.i0 + lane];
            const int bucket = a.bucket[r.i0 + lane];
            mine_ok = bucket >= -1 && bucket < a.G && h.flt_begin >= 0 && h.fix_begin >= 0 &&
                      static_cast<int64_t>(h.flt_begin) + h.n_flt <= a.n_flt && static_cast<int64_t>(h.fix_begin) + h.n_fix <= a.n_fix;
        }
        // a bucket or a leg range that cannot be right: nothing of the chunk is read, its record is NaN (the cell's own)
        const bool ok = __ballot(!mine_ok) == 0;
        Sums s{0.0, 0.0, 0.0};
        if (cnt > 0 && ok) {
            const int l_begin = scen::lane_int(h.flt_begin, 0), l_end = scen::lane_int(h.flt_begin + h.n_flt, cnt - 1);
            for (int base = l_begin; base < l_end; base += kWave) {
                const int f = base + lane;
                const int j = owner_lane(h.flt_begin, cnt, f);
                const TradeRef t = owner_trade(h, j);
                const double zt = __shfl(z, j, kWave);
                if (f < l_end) {
                    Amount3 pay, start;
                    float_nodes(g, a.tau, t, zt, static_cast<int>(f - t.l0), &pay, &start);
                    add_node<kLog, kGamma>(pay, s_x, s_comp, s_log, K, Kc, method, tab, s);
                    add_node<kLog, kGamma>(start, s_x, s_comp, s_log, K, Kc, method, tab, s);
                }
            }
            const int x_begin = scen::lane_int(h.fix_begin, 0), x_end = scen::lane_int(h.fix_begin + h.n_fix, cnt - 1);
            for (int base = x_begin; base < x_end; base += kWave) {
                const int f = base + lane;
                const int j = owner_lane(h.fix_begin, cnt, f);
                const TradeRef t = owner_trade(h, j);
                const double zt = __shfl(z, j, kWave);
                if (f < x_end)
                    add_node<kLog, kGamma>(fixed_node(g, a.tau, t, zt, static_cast<int>(f - t.f0)), s_x, s_comp, s_log, K, Kc, method, tab, s);
            }
        }
        s.pv = wave_sum(s.pv);
        s.cs = wave_sum(s.cs);
        if (kGamma) s.csg = wave_sum(s.csg);
        wave_lds_order();
        double* rec = a.work + ch * a.S;
        if (lane == 0) {
            rec[0] = ok ? s.pv : NAN;
            rec[1 + NT * Kc] = ok ? s.cs : NAN;
            if (kGamma) rec[2 + NT * Kc] = ok ? s.csg : NAN;
        }
        for (int k = lane; k < NT * Kc; k += kWave) {
            rec[1 + k] = ok ? tab[k] : NAN;
            tab[k] = 0.0;
        }
        wave_lds_order();
    }
}

struct ProjectArgs {
    CurveDev cv;
    const double* sums;              // [B][S] the desks' sums
    const double* cells;             // [C][S] the cells' sums
    int S, G;
    int64_t B, C;
    const int64_t* desk_cell_off;    // [B + 1]
    const int32_t* cell_bucket;      // [C]
    int want_delta, want_gamma;
    double* out;                     // [B][1 + Q + Q Q]
};

// The curve block of the augmented ladder from the desks' sums and +0.0 in every spread row and column.
__global__ __launch_bounds__(kWave * kProjWaves) void credit_project_kernel(ProjectArgs a) { project_curve_block<true>(a); }

// The spread rows and columns from the cells' sums, one wave per cell; every value is computed once and written where it
// belongs (twice for the cross terms, sbl::cross_sum).  Runs after credit_project_kernel on the same stream.
__global__ __launch_bounds__(kWave * kCellWaves) void credit_cell_kernel(ProjectArgs a) {
    const CurveDev& cv = a.cv;
    const int P = cv.P, Kc = cv.Kc, Q = P + a.G;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kCellWaves + wave;
    if (j >= a.C) return;
    const int g = a.cell_bucket[j];                      // uniform: scalar loads
    if (g < 0 || g >= a.G) return;
    int64_t lo = 0, hi = a.B;                            // the desk of cell j: the last b with desk_cell_off[b] <= j
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (a.desk_cell_off[mid] <= j) lo = mid;
        else hi = mid;
    }
    const int64_t stride = 1 + Q + static_cast<int64_t>(Q) * Q;
    double* row = a.out + lo * stride;
    const double* rec = a.cells + j * a.S;
    const int nt = a.want_gamma ? 4 : 1;
    if (a.want_delta && lane == 0) row[1 + P + g] = rec[1 + nt * Kc] * 1e-4;
    if (!a.want_gamma) return;
    double* gamma = row + 1 + Q;
    if (lane == 0) gamma[static_cast<int64_t>(P + g) * Q + P + g] = rec[2 + nt * Kc] * 1e-8;
    const double* wz = rec + 1 + 3 * Kc;
    for (int p = lane; p < P; p += kWave) {
        const double v = cross_sum(wz, Kc, [&](int k) { return lj_at(cv, k, p); }) * 1e-8;
        gamma[static_cast<int64_t>(p) * Q + P + g] = v;
        gamma[static_cast<int64_t>(P + g) * Q + p] = v;
    }
}

// -------------------------------------------------------------------------------------------------------------- host
struct Extra {           // what the trades carry besides the batch
    const double* z;
    const int32_t* bucket;
    int64_t n_fix;
    const double* fix_tau;
    int64_t n_flt;
    const double* flt_tau;
    int G;
};

int check_buckets(const std::string& w, int G) {
    if (G < 0 || G > ADR_CREDIT_MAX_BUCKETS)
        return adr_set_error(ADR_ERR_INVALID, w + ": 0 .. ADR_CREDIT_MAX_BUCKETS (32) spread buckets are allowed");
    return ADR_OK;
}

// The scalars and handles of an entry, checked.
int handles(const std::string& w, const adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, const Extra& x, int64_t B,
            const Request& rq, Handles* h) {
    int rc = check_handles(w, ctx, curve, trades, B, h);
    if (rc == ADR_OK) rc = check_buckets(w, x.G);
    if (rc != ADR_OK) return rc;
    if (!x.z || !x.bucket) return adr_set_error(ADR_ERR_INVALID, w + ": z or bucket is NULL");
    if (x.n_fix < 0 || x.n_flt < 0 || x.n_fix > INT32_MAX || x.n_flt > INT32_MAX)
        return adr_set_error(ADR_ERR_INVALID, w + ": flow counts must lie in 0 .. 2^31 - 1");
    if ((x.n_fix > 0 && !x.fix_tau) || (x.n_flt > 0 && !x.flt_tau)) return adr_set_error(ADR_ERR_INVALID, w + ": null spread-time array");
    return check_fit(w, trades, *h, rq, tables(rq.gamma));
}

// The spread side on the host: finite z and spread times, buckets inside -1 .. G - 1 (credit_scenario_pv.hip's wording).
int check_spreads(const std::string& w, int64_t n, const Extra& x) {
    for (int64_t i = 0; i < n; ++i) {
        if (!std::isfinite(x.z[i])) return adr_set_error(ADR_ERR_INVALID, w + ": spreads z must be finite (trade " + std::to_string(i) + ")");
        if (x.bucket[i] < -1 || x.bucket[i] >= x.G)
            return adr_set_error(ADR_ERR_INVALID, w + ": bucket " + std::to_string(x.bucket[i]) + " of trade " + std::to_string(i) +
                                                      " is outside -1 .. G - 1");
    }
    for (int64_t i = 0; i < x.n_fix; ++i)
        if (!std::isfinite(x.fix_tau[i])) return adr_set_error(ADR_ERR_INVALID, w + ": spread times must be finite (fixed flow " + std::to_string(i) + ")");
    for (int64_t i = 0; i < x.n_flt; ++i)
        if (!std::isfinite(x.flt_tau[i])) return adr_set_error(ADR_ERR_INVALID, w + ": spread times must be finite (float coupon " + std::to_string(i) + ")");
    return ADR_OK;
}

struct Cells {           // the (desk, bucket) cells of an ordered batch: only those that hold trades
    std::vector<int64_t> cell_off, desk_cell_off;        // [C + 1] trades, [B + 1] cells
    std::vector<int32_t> cell_bucket;                    // [C]
    int64_t count() const { return static_cast<int64_t>(cell_bucket.size()); }
};

// sub_off and the buckets (already checked against G) cut into cells; a desk whose buckets decrease is refused.
int build_cells(const std::string& w, int64_t n, int64_t B, const int64_t* sub_off, const int32_t* bucket, Cells& c) {
    const int rc = sub::check_offsets(w, n, B, sub_off);
    if (rc != ADR_OK) return rc;
    c.cell_off.clear();
    c.desk_cell_off.assign(1, 0);
    c.cell_bucket.clear();
    for (int64_t b = 0; b < B; ++b) {
        for (int64_t i = sub_off[b]; i < sub_off[b + 1]; ++i) {
            if (i > sub_off[b] && bucket[i] < bucket[i - 1])
                return adr_set_error(ADR_ERR_INVALID, w + ": sub-book " + std::to_string(b) + " is not ordered by bucket: trade " +
                                                          std::to_string(i) + " (bucket " + std::to_string(bucket[i]) +
                                                          ") follows bucket " + std::to_string(bucket[i - 1]));
            if (i == sub_off[b] || bucket[i] != bucket[i - 1]) {
                c.cell_off.push_back(i);
                c.cell_bucket.push_back(bucket[i]);
            }
        }
        c.desk_cell_off.push_back(c.count());
    }
    c.cell_off.push_back(n);
    return ADR_OK;
}

// The device pointers of one call.
struct DevArrays {
    Extra x;
    int64_t C;
    const int64_t *cell_plan, *desk_cell_off;
    const int32_t* cell_bucket;
};

int64_t work_doubles(int Kc, int64_t n, int64_t B, int64_t C, bool gamma, int64_t* chunks) {
    const int64_t cap = sub::max_chunks(n, C, kChunk);
    if (chunks) *chunks = cap;
    return (cap + C + B) * record_doubles(Kc, gamma);
}

// The chain on `stream`; every pointer is device memory.  work: adr_credit_subbook_ladders_work doubles, laid out as the
// chunk records [cap][S], the cells' sums [C][S] and the desks' sums [B][S].
int enqueue(const std::string& w, adr_ctx* ctx, const Handles& h, int64_t B, const DevArrays& d, const Request& rq, double* out,
            double* work, hipStream_t stream_or_null) {
    if (d.C < 1 || d.C > h.tr->n) return adr_set_error(ADR_ERR_INVALID, w + ": the cell count must lie in 1 .. the trade count");
    if (!d.cell_plan) return adr_set_error(ADR_ERR_INVALID, w + ": the cell plan is NULL (adr_scenario_subbook_plan over the cells fills it)");
    if (!d.desk_cell_off || !d.cell_bucket) return adr_set_error(ADR_ERR_INVALID, w + ": desk_cell_off or cell_bucket is NULL");
    if (!out) return adr_set_error(ADR_ERR_INVALID, w + ": out is NULL");
    if (!work) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_credit_subbook_ladders_work doubles are needed)");
    hipStream_t stream = nullptr;
    const int rc = call::target_stream(w, ctx, stream_or_null, &stream);
    if (rc != ADR_OK) return rc;
    const CurveDev& cv = *h.cv;
    const int S = record_doubles(cv.Kc, rq.gamma);
    const int64_t C = d.C, cap = sub::max_chunks(h.tr->n, C, kChunk);
    const sub::Plan pl = sub::plan_view(d.cell_plan, C);
    double *cells = work + cap * S, *sums = cells + C * S;
    const KnotGrid kg = knot_grid(ctx, cv, tables(rq.gamma), cap);
    const KnotArgs ka{cv, *h.tr, d.x.z, d.x.bucket, Taus{d.x.fix_tau, d.x.flt_tau}, d.x.n_fix, d.x.n_flt, d.x.G, cap, pl.chunk_off + C,
                      pl.bounds, work, S, kg.waves};
    const bool is_log = cv.method != ADR_INTERP_LINEAR_FWD_RATES;
    hipError_t e = launch_knot(rq.gamma ? (is_log ? &credit_subbook_knot_kernel<true, true> : &credit_subbook_knot_kernel<false, true>)
                                        : (is_log ? &credit_subbook_knot_kernel<true, false> : &credit_subbook_knot_kernel<false, false>),
                               ka, kg, stream);
    if (e == hipSuccess) e = sub::enqueue_sum(work, pl.chunk_off, cap, C, S, cells, stream);
    if (e == hipSuccess) e = sub::enqueue_sum(cells, d.desk_cell_off, C, B, S, sums, stream);
    const int64_t tiles = (B + kProjDesks - 1) / kProjDesks, cell_blocks = (C + kCellWaves - 1) / kCellWaves;
    if (e == hipSuccess && (tiles > INT32_MAX || cell_blocks > INT32_MAX)) e = hipErrorInvalidConfiguration;
    if (e == hipSuccess) {
        const ProjectArgs pa{cv, sums, cells, S, d.x.G, B, C, d.desk_cell_off, d.cell_bucket, rq.delta ? 1 : 0, rq.gamma ? 1 : 0, out};
        hipLaunchKernelGGL(credit_project_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(cv.P + d.x.G + 1)),
                           dim3(kWave * kProjWaves), 0, stream, pa);
        e = hipGetLastError();
        if (e == hipSuccess && d.x.G > 0 && rq.delta) {
            hipLaunchKernelGGL(credit_cell_kernel, dim3(static_cast<unsigned>(cell_blocks)), dim3(kWave * kCellWaves), 0, stream, pa);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// The chunks [lo, hi) of the cell plan on the host: work[ch] = the chunk's record.
template <bool kLog>
void host_chunks(const CurveTables& t, int method, bool gamma, const scen::HostBatch& b, const Extra& x, const int64_t* bounds, int S,
                 double* work, int64_t lo, int64_t hi) {
    const int K = t.K, Kc = t.Kc, nt = tables(gamma);
    const Flows g{b.fix_tp, b.fix_pay, b.flt_tp, b.flt_ts, b.flt_te, b.flt_alpha};
    const Taus u{x.fix_tau, x.flt_tau};
    for (int64_t ch = lo; ch < hi; ++ch) {
        double* rec = work + ch * S;
        std::fill(rec, rec + S, 0.0);
        double &cs = rec[1 + nt * Kc], &csg = rec[S - 1];        // (without GAMMA csg is cs's slot and is not formed)
        auto add = [&](const Amount3& n) {
            if (!n.on) return;
            const DateW d = lookup<kLog>(n.t, t.x.data(), K, method, t.compact_of.data());
            const Factor e = node_factor<kLog>(d, t.log_df.data());
            const Terms v = node_terms_at<kLog>(d, n.a, e), v1 = node_terms_at<kLog>(d, n.a1, e);
            const bool two = d.b != d.a;
            rec[0] = rec[0] + v.pv;
            cs = cs + v1.pv;
            rec[1 + d.a] = rec[1 + d.a] + v.wa;
            if (two) rec[1 + d.b] = rec[1 + d.b] + v.wb;
            if (!gamma) return;
            csg = csg + node_terms_at<kLog>(d, n.a2, e).pv;
            rec[1 + Kc + d.a] = rec[1 + Kc + d.a] + v.da;
            if (two) {
                rec[1 + Kc + d.b] = rec[1 + Kc + d.b] + v.db;
                if (kLog) rec[1 + 2 * Kc + d.a] = rec[1 + 2 * Kc + d.a] + v.o;
            }
            rec[1 + 3 * Kc + d.a] = rec[1 + 3 * Kc + d.a] + v1.wa;
            if (two) rec[1 + 3 * Kc + d.b] = rec[1 + 3 * Kc + d.b] + v1.wb;
        };
        host_chunk_walk(
            b, bounds, ch,
            [&](const TradeRef& tr, int64_t i, int c) {
                Amount3 pay, start;
                float_nodes(g, u, tr, x.z[i], c, &pay, &start);
                add(pay);
                add(start);
            },
            [&](const TradeRef& tr, int64_t i, int c) { add(fixed_node(g, u, tr, x.z[i], c)); });
    }
}

// out[b] of the desks [lo, hi) from their sums and their cells' sums: the two kernels' expressions and orders.
void host_project(const CurveTables& t, const Request& rq, int G, const double* sums, const double* cells, const Cells& c, int S,
                  double* out, int64_t lo, int64_t hi) {
    const int P = t.P, Kc = t.Kc, Q = P + G;
    const size_t stride = 1 + Q + static_cast<size_t>(Q) * Q;
    const int nt = tables(rq.gamma);
    for (int64_t b = lo; b < hi; ++b) {
        double *o = out + b * stride, *gamma = o + 1 + Q;
        host_project_curve(t, rq, sums + b * S, Q, o);
        for (int64_t j = c.desk_cell_off[b]; rq.delta && j < c.desk_cell_off[b + 1]; ++j) {
            const int g = c.cell_bucket[j];
            if (g < 0) continue;
            const double* cell = cells + j * S;
            o[1 + P + g] = cell[1 + nt * Kc] * 1e-4;
            if (!rq.gamma) continue;
            gamma[static_cast<size_t>(P + g) * Q + P + g] = cell[2 + nt * Kc] * 1e-8;
            const double* wz = cell + 1 + 3 * Kc;
            for (int p = 0; p < P; ++p) {
                const double v = cross_sum(wz, Kc, [&](int k) { return host_lj(t, k, p); }) * 1e-8;
                gamma[static_cast<size_t>(p) * Q + P + g] = v;
                gamma[static_cast<size_t>(P + g) * Q + p] = v;
            }
        }
    }
}

}  // namespace csl
}  // namespace adr

namespace CL = adr::csl;

extern "C" {

int64_t adr_credit_subbook_ladders_work(const adr_curve* curve, int64_t n, int64_t B, int64_t C, uint32_t req_mask, int64_t* chunks) {
    const adr_ctx* owner = nullptr;
    const adr::CurveDev* cv = adr_curve_device_view(curve, &owner);
    if (!cv || n < 1 || B < 1 || C < 1 || C > n) return 0;
    return CL::work_doubles(cv->Kc, n, B, C, CL::request_of(req_mask).gamma, chunks);
}

int adr_credit_subbook_ladders_dev(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, const double* z_dev,
                                   const int32_t* bucket_dev, int64_t n_fix, const double* fix_tau_dev, int64_t n_flt,
                                   const double* flt_tau_dev, int G, int64_t B, int64_t C, const int64_t* cell_plan_dev,
                                   const int64_t* desk_cell_off_dev, const int32_t* cell_bucket_dev, uint32_t req_mask,
                                   double* out_dev, double* work_dev, void* stream) {
    const std::string w = "adr_credit_subbook_ladders_dev";
    const CL::Request rq = CL::request_of(req_mask);
    const CL::Extra x{z_dev, bucket_dev, n_fix, fix_tau_dev, n_flt, flt_tau_dev, G};
    CL::Handles h{};
    const int rc = CL::handles(w, ctx, curve, trades, x, B, rq, &h);
    if (rc != ADR_OK) return rc;
    const CL::DevArrays d{x, C, cell_plan_dev, desk_cell_off_dev, cell_bucket_dev};
    return CL::enqueue(w, ctx, h, B, d, rq, out_dev, work_dev, static_cast<hipStream_t>(stream));
}

int adr_credit_subbook_ladders(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, const double* z, const int32_t* bucket,
                               int64_t n_fix, const double* fix_tau, int64_t n_flt, const double* flt_tau, int G, int64_t B,
                               const int64_t* sub_off, uint32_t req_mask, double* out) {
    const std::string w = "adr_credit_subbook_ladders";
    const CL::Request rq = CL::request_of(req_mask);
    const CL::Extra x{z, bucket, n_fix, fix_tau, n_flt, flt_tau, G};
    CL::Handles h{};
    int rc = CL::handles(w, ctx, curve, trades, x, B, rq, &h);
    if (rc != ADR_OK) return rc;
    if (!out) return adr_set_error(ADR_ERR_INVALID, w + ": out is NULL");
    const int64_t n = h.tr->n;
    rc = CL::check_spreads(w, n, x);
    if (rc != ADR_OK) return rc;
    CL::Cells cells;
    rc = CL::build_cells(w, n, B, sub_off, bucket, cells);
    if (rc != ADR_OK) return rc;
    const int64_t C = cells.count();
    std::vector<int64_t> plan;
    rc = adr::sub::build_plan(w, n, C, cells.cell_off.data(), plan);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const int Q = h.cv->P + G;
    double *dout, *dwork, *dz, *dft, *dlt;
    int64_t *dplan, *ddesk;
    int32_t *dbucket, *dcellb;
    adr::call::Staging mem;                         // `plan` and `cells` are uploaded from where they stand: they outlive finish()
    mem.out(&dout, out, static_cast<size_t>(B) * (1 + Q + static_cast<size_t>(Q) * Q));
    mem.scratch(&dwork, static_cast<size_t>(CL::work_doubles(h.cv->Kc, n, B, C, rq.gamma, nullptr)));
    mem.in(&dz, z, n);
    mem.in(&dft, fix_tau, n_fix);
    mem.in(&dlt, flt_tau, n_flt);
    mem.in(&dplan, plan.data(), plan.size());
    mem.in(&ddesk, cells.desk_cell_off.data(), B + 1);
    mem.in(&dbucket, bucket, n);
    mem.in(&dcellb, cells.cell_bucket.data(), C);
    const hipError_t e = mem.begin(stream);
    const CL::DevArrays da{CL::Extra{dz, dbucket, n_fix, dft, n_flt, dlt, G}, C, dplan, ddesk, dcellb};
    if (e == hipSuccess) rc = CL::enqueue(w, ctx, h, B, da, rq, dout, dwork, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_credit_subbook_ladders_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac,
                                    const double* hess, int64_t n, const int64_t* fix_off, const int64_t* flt_off,
                                    const double* fix_tp, const double* fix_pay, const double* flt_tp, const double* flt_ts,
                                    const double* flt_te, const double* flt_alpha, const double* flt_weight, const double* notional,
                                    const double* spread, const double* fix_sign, const double* flt_sign, const double* z,
                                    const int32_t* bucket, const double* fix_tau, const double* flt_tau, int G, int64_t B,
                                    const int64_t* sub_off, uint32_t req_mask, double* out) {
    const std::string w = "adr_credit_subbook_ladders_host";
    namespace SC = adr::scen;
    const CL::Request rq = CL::request_of(req_mask);
    const CL::HostCurve c{interp_method, K, P, times, dfs, jac, hess};
    const SC::HostBatch b{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, flt_weight, notional, spread,
                          fix_sign, flt_sign};
    int rc = CL::check_host_counts(w, interp_method, n, B);
    if (rc == ADR_OK) rc = CL::check_buckets(w, G);
    if (rc == ADR_OK) rc = CL::check_host_arrays(w, c, b, rq, out);
    if (rc != ADR_OK) return rc;
    if (!z || !bucket) return adr_set_error(ADR_ERR_INVALID, w + ": z or bucket is NULL");
    rc = CL::check_host_trades(w, b);
    if (rc != ADR_OK) return rc;
    const CL::Extra x{z, bucket, fix_off[n], fix_tau, flt_off[n], flt_tau, G};
    if ((x.n_fix > 0 && !fix_tau) || (x.n_flt > 0 && !flt_tau)) return adr_set_error(ADR_ERR_INVALID, w + ": null spread-time array");
    rc = CL::check_spreads(w, n, x);
    if (rc != ADR_OK) return rc;
    CL::Cells cells;
    rc = CL::build_cells(w, n, B, sub_off, bucket, cells);
    if (rc != ADR_OK) return rc;
    const int64_t C = cells.count();
    std::vector<int64_t> plan;
    rc = adr::sub::build_plan(w, n, C, cells.cell_off.data(), plan);
    if (rc != ADR_OK) return rc;
    adr::CurveTables t;
    rc = CL::host_tables(w, c, b, rq, t);
    if (rc != ADR_OK) return rc;
    const int S = CL::record_doubles(t.Kc, rq.gamma);
    const int64_t chunks = plan[C];
    std::vector<double> work(static_cast<size_t>(chunks) * S), csum(static_cast<size_t>(C) * S), sums(static_cast<size_t>(B) * S);
    const int64_t* bounds = plan.data() + C + 1;
    const bool lin = interp_method == ADR_INTERP_LINEAR_FWD_RATES;
    adr::parallel_ranges(chunks, adr::pool_threads(chunks, 4), [&](int, int64_t lo, int64_t hi) {
        if (lin) CL::host_chunks<false>(t, interp_method, rq.gamma, b, x, bounds, S, work.data(), lo, hi);
        else CL::host_chunks<true>(t, interp_method, rq.gamma, b, x, bounds, S, work.data(), lo, hi);
    });
    adr::sub::reduce_subbooks(work.data(), plan.data(), C, S, csum.data());
    adr::sub::reduce_subbooks(csum.data(), cells.desk_cell_off.data(), B, S, sums.data());
    adr::parallel_ranges(B, adr::pool_threads(B, 1), [&](int, int64_t lo, int64_t hi) {
        CL::host_project(t, rq, G, sums.data(), csum.data(), cells, S, out, lo, hi);
    });
    return ADR_OK;
}

}  // extern "C"
