// Inflation sub-book Greeks: per-desk PV, discount delta and gamma, breakeven delta and gamma and the discount x
// breakeven cross gamma of one YoY book from ONE launch chain (adr_yoy_subbook_ladders*; declarations and semantics:
// include/adrates.h).
//
// A YoY coupon pays amount = scale (1 + y - 1 + spread) at tp and its amount does not depend on the discount curve, so on
// the discount side it is a fixed flow: the knot-space node of subbook_ladder.hip (`fixed_node` rules, tp > 0 live).  On
// the inflation side it is yoy_risk.hip's coupon (yoy_nodes.hpp): with E = D(tp) as the knot tables give it and
// g = scale (1 + y) E it adds g u_k to the breakeven delta and g (u_k u_l + [k == l] v_k) to the breakeven gamma over its
// at most four live slots.  The mixed derivative is the product of the two: a node is linear in its amount in all three
// discount schemes, so with t the node of the UNIT amount at tp the coupon adds
//     M[a][k] += scale (1 + y) u_k t.wa   at compact knot d.a,   and the same with t.wb at d.b,
// and gamma'[p][P_d + k] = 1e-8 sum_a M[a][k] LJ[a][p] (sbl::cross_sum, as the credit cells' spread table).
//
//   1. yoy_subbook_knot_kernel: one wave per chunk of the sub-book plan (at most 64 consecutive swaps of ONE desk), lane =
//      flow, 64 at a time over the chunk's contiguous run of fixed flows and then over its run of coupons.  A flow carries
//      everything it needs (the YoY arrays hold signed amounts per flow, nothing per swap), so there is no owner search.
//      Wavefront-scope LDS adds into the wave's tables [w, D, O, di, gi, M] ([w, di] without GAMMA);
//      work[chunk] = [pv, tables].
//   2. sub::enqueue_sum adds every desk's chunk records.
//   3. yoy_project_kernel writes pv and the discount block of out[b] = [pv, delta'[Q], gamma'[Q][Q]], Q = P_d + P_i, from the
//      desk sums (sbl::project_curve_block, subbook_ladder.hip's code) and +0.0 elsewhere; yoy_infl_kernel then writes the
//      breakeven delta and gamma and the cross block, each cross value computed once and stored twice.
//
// E carries no division by D(0): adr_yoy_risk divides by it, and the two agree where D(0) == 1.0, which holds on every curve
// the engine builds.  The host twin (adr_yoy_subbook_ladders_host) runs the same node, sum and projection code in the
// same chunks and orders on the CPU.
#include "subbook_ladder_common.hpp"
#include "yoy_nodes.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace ysl {

using namespace sbl;     // the shared pieces (subbook_ladder_common.hpp)

constexpr int kDeskWaves = 4;       // desks per block of the inflation kernel, one wave each

// ---------------------------------------------------------------------------------------------------- nodes (shared)
struct Book {            // a YoY book as adr_yoy_scenario_subbook_pv takes it
    int64_t n, n_fix, m;
    const int64_t* fix_off;
    const double *fix_tp, *fix_pay;
    const int64_t* cpn_off;
    const double* cpn;
};

struct InflCurve {
    int method, P;
    const double *T, *b;
};

// A wave's tables, and a record after its pv: w, D, O [Kc], di [P_i], gi [P_i][P_i], M [P_i][Kc]; without GAMMA w, di.
struct Layout {
    int Kc, Pi;
    bool gamma;
    __host__ __device__ int di() const { return gamma ? 3 * Kc : Kc; }
    __host__ __device__ int gi() const { return di() + Pi; }
    __host__ __device__ int M() const { return gi() + Pi * Pi; }
    __host__ __device__ int size() const { return gamma ? M() + Pi * Kc : gi(); }
};

inline int record_doubles(int Kc, int Pi, bool gamma) { return 1 + Layout{Kc, Pi, gamma}.size(); }

// A discount node's numbers into the tables w, D, O: subbook_ladder.hip's adds in its order.
template <bool kLog, class Add>
__host__ __device__ inline void add_discount(const DateW& d, const Terms& t, int Kc, bool gamma, const Add& add, double& pv) {
    const bool two = d.b != d.a;
    pv = pv + t.pv;
    add(d.a, t.wa);
    if (two) add(d.b, t.wb);
    if (!gamma) return;
    add(Kc + d.a, t.da);
    if (two) {
        add(Kc + d.b, t.db);
        if (kLog) add(2 * Kc + d.a, t.o);
    }
}

// Fixed flow f: counts when tp > 0 and it pays something (sbl::fixed_node on a batch without float coupons).
template <bool kLog, class Comp, class Add>
__host__ __device__ inline void add_fixed(const Book& bk, int64_t f, const double* x, int K, int method, const Comp* comp,
                                          const double* L, const Layout& y, const Add& add, double& pv) {
    const double tp = bk.fix_tp[f], pay = bk.fix_pay[f];
    if (!(tp > 0.0) || pay == 0.0) return;
    const DateW d = lookup<kLog>(tp, x, K, method, comp);
    add_discount<kLog>(d, node_terms<kLog>(d, pay, L), y.Kc, y.gamma, add, pv);
}

// YoY coupon i on both curves.  c on the unit grid: c.g = scale (1 + y).
template <bool kLog, class Comp, class Add>
__host__ __device__ inline void add_coupon(const Book& bk, int64_t i, const double* unit, const yoy::Infl& f, const double* x,
                                           int K, int method, const Comp* comp, const double* L, const Layout& y, const Add& add,
                                           double& pv) {
    const yoy::Desc c = yoy::describe(unit, unit + 2, 2, ADR_INTERP_LINEAR_FWD_RATES, 1.0, f, bk.cpn, bk.m, i);
    const double tp = bk.cpn[ADR_YOY_TP * bk.m + i];
    if (!(tp > 0.0)) return;                                    // a dead coupon: nothing on either curve
    const DateW d = lookup<kLog>(tp, x, K, method, comp);
    const Factor e = node_factor<kLog>(d, L);
    const Terms t = node_terms_at<kLog>(d, 1.0, e);             // the unit amount at tp: t.pv = E
    if (c.amount != 0.0) add_discount<kLog>(d, node_terms_at<kLog>(d, c.amount, e), y.Kc, y.gamma, add, pv);
    const double g = c.g * t.pv;
    const bool two = d.b != d.a;
    const int di = y.di(), gi = y.gi(), M = y.M();
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int kp = c.k[p] - 1;
        if (kp < 0) continue;
        add(di + kp, g * c.u[p]);
        if (!y.gamma) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (c.k[q] > 0) add(gi + kp * y.Pi + (c.k[q] - 1), g * yoy::gamma_term(c.u[p], c.u[q], c.v[p], p == q));
        const double s = c.g * c.u[p];
        add(M + kp * y.Kc + d.a, s * t.wa);
        if (two) add(M + kp * y.Kc + d.b, s * t.wb);
    }
}

// The breakeven block and the cross block of one desk's row from its sums rec (after pv), each value computed once:
// lj(a, p) = LJ[a][p].  Entry e of [e0, e1) in steps of `step`; the blocks the request leaves out stay as they are.
template <class LJ>
__host__ __device__ inline void project_inflation(const double* rec, const Layout& y, int P, bool want_delta, double* row, int e0,
                                                  int step, const LJ& lj) {
    const int Pi = y.Pi, Q = P + Pi;
    if (!want_delta) return;
    for (int k = e0; k < Pi; k += step) row[1 + P + k] = rec[y.di() + k] * 1e-4;
    if (!y.gamma) return;
    double* gamma = row + 1 + Q;
    for (int e = e0; e < Pi * Pi; e += step) gamma[static_cast<int64_t>(P + e / Pi) * Q + P + e % Pi] = rec[y.gi() + e] * 1e-8;
    for (int e = e0; e < Pi * P; e += step) {
        const int k = e / P, p = e % P;
        const double v = cross_sum(rec + y.M() + k * y.Kc, y.Kc, [&](int a) { return lj(a, p); }) * 1e-8;
        gamma[static_cast<int64_t>(p) * Q + P + k] = v;
        gamma[static_cast<int64_t>(P + k) * Q + p] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------ device
struct KnotArgs {
    CurveDev cv;
    Book bk;
    InflCurve ic;
    int64_t chunk_cap;               // the rows `work` holds, an upper bound of the plan's count
    const int64_t *sub_chunks, *sub_bounds;      // the plan's chunk count and its [chunks][2] swap bounds (subbook.hpp)
    double* work;                    // [chunk_cap][S]
    int S, waves;
};

__device__ inline double wave_sum(double v) {
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, kWave);
    return v;
}

struct LdsAdd {          // one entry of the wave's tables
    double* tab;
    // As subbook_ladder.hip: the bit contract rests on the order in which the hardware applies the adds of ONE instruction
    // to the same address, which is fixed by the lane ids - observed behaviour of ds_add_f64 on gfx950, not a guarantee.
    __device__ void operator()(int i, double v) const {
        __hip_atomic_fetch_add(tab + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
};

// The doubles a block keeps beside its waves' tables and the knot arrays of sbl::shared_bytes: the inflation nodes
// x, L, L', L'' [P_i + 1] and the unit grid.
inline size_t infl_doubles(int Pi) { return 4 * (static_cast<size_t>(Pi) + 1) + 4; }

template <bool kLog, bool kGamma>
__global__ __launch_bounds__(kWave * kMaxWaves) void yoy_subbook_knot_kernel(KnotArgs a) {
    extern __shared__ double lds[];
    const int K = a.cv.K, Kc = a.cv.Kc, Pi = a.ic.P, N = Pi + 1, waves = a.waves;
    const Layout y{Kc, Pi, kGamma};
    const int TW = y.size();
    double* s_tab = lds;                                 // [waves][TW]
    double* s_x = s_tab + waves * TW;                    // [K]
    double* s_log = s_x + K;                             // [Kc]
    double* s_ix = s_log + Kc;                           // [N] each: the inflation nodes
    double *s_L = s_ix + N, *s_L1 = s_L + N, *s_L2 = s_L1 + N;
    double* s_unit = s_L2 + N;                           // [4]
    int16_t* s_comp = reinterpret_cast<int16_t*>(s_unit + 4);      // [K]
    const int threads = kWave * waves;
    for (int i = threadIdx.x; i < waves * TW; i += threads) s_tab[i] = 0.0;
    for (int i = threadIdx.x; i < K; i += threads) {
        s_x[i] = a.cv.x[i];
        s_comp[i] = a.cv.compact_of[i];
    }
    for (int i = threadIdx.x; i < Kc; i += threads) s_log[i] = a.cv.log_df[i];
    for (int k = threadIdx.x; k < N; k += threads) yoy::make_node(a.ic.T, a.ic.b, k, s_ix + k, s_L + k, s_L1 + k, s_L2 + k);
    if (threadIdx.x == 0) {
        s_unit[0] = yoy::kUnitX[0]; s_unit[1] = yoy::kUnitX[1];
        s_unit[2] = yoy::kUnitD[0]; s_unit[3] = yoy::kUnitD[1];
    }
    __syncthreads();

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    double* tab = s_tab + wave * TW;
    const LdsAdd add{tab};
    const yoy::Infl f{s_ix, s_L, s_L1, s_L2, N, a.ic.method};
    const Book& bk = a.bk;
    const int method = a.cv.method;
    int64_t n_chunks = *a.sub_chunks;                    // uniform: a scalar load
    n_chunks = n_chunks < a.chunk_cap ? n_chunks : a.chunk_cap;
    for (int64_t ch = static_cast<int64_t>(blockIdx.x) * waves + wave; ch < n_chunks; ch += static_cast<int64_t>(gridDim.x) * waves) {
        scen::ChunkRange r = scen::chunk_range<true>(ch, a.sub_bounds, bk.n);
        if (r.i1 > r.i0 + kChunk) r.i1 = r.i0 + kChunk;  // (a plan of build_plan never asks for more)
        const int cnt = r.i1 > r.i0 ? static_cast<int>(r.i1 - r.i0) : 0;
        int f_lo = 0, f_hi = 0, c_lo = 0, c_hi = 0;
        bool mine_ok = true;
        if (lane < cnt) {
            const int64_t i = r.i0 + lane;
            const int64_t fl = bk.fix_off[i], fh = bk.fix_off[i + 1], cl = bk.cpn_off[i], chi = bk.cpn_off[i + 1];
            mine_ok = fl >= 0 && fh >= fl && fh <= bk.n_fix && cl >= 0 && chi >= cl && chi <= bk.m;
            f_lo = static_cast<int>(fl); f_hi = static_cast<int>(fh);        // (the totals fit an int)
            c_lo = static_cast<int>(cl); c_hi = static_cast<int>(chi);
        }
        // a leg range that cannot be right: nothing of the chunk is read, its record is NaN (the desk's own).  With every
        // lane's range right the chunk's flows are the runs from lane 0's begin to lane cnt - 1's end.
        const bool ok = __ballot(!mine_ok) == 0;
        double pv = 0.0;
        if (cnt > 0 && ok) {
            const int64_t f0 = scen::lane_int(f_lo, 0), f1 = scen::lane_int(f_hi, cnt - 1);
            for (int64_t base = f0; base < f1; base += kWave)
                if (base + lane < f1) add_fixed<kLog>(bk, base + lane, s_x, K, method, s_comp, s_log, y, add, pv);
            const int64_t c0 = scen::lane_int(c_lo, 0), c1 = scen::lane_int(c_hi, cnt - 1);
            for (int64_t base = c0; base < c1; base += kWave)
                if (base + lane < c1) add_coupon<kLog>(bk, base + lane, s_unit, f, s_x, K, method, s_comp, s_log, y, add, pv);
        }
        pv = wave_sum(pv);
        wave_lds_order();
        double* rec = a.work + ch * a.S;
        if (lane == 0) rec[0] = ok ? pv : NAN;
        for (int k = lane; k < TW; k += kWave) {
            rec[1 + k] = ok ? tab[k] : NAN;
            tab[k] = 0.0;
        }
        wave_lds_order();
    }
}

struct ProjectArgs {
    CurveDev cv;
    const double* sums;              // [B][S] the desks' sums
    int S, G;                        // G = P_i: the columns past the discount pillars
    int64_t B;
    int want_delta, want_gamma;
    double* out;                     // [B][1 + Q + Q Q]
};

// pv and the discount block of the augmented ladder from the desks' sums and +0.0 in every breakeven row and column.
__global__ __launch_bounds__(kWave * kProjWaves) void yoy_project_kernel(ProjectArgs a) { project_curve_block<true>(a); }

// The breakeven rows and columns from the desks' sums, one wave per desk.  Runs after yoy_project_kernel on the same
// stream.
__global__ __launch_bounds__(kWave * kDeskWaves) void yoy_infl_kernel(ProjectArgs a) {
    const CurveDev& cv = a.cv;
    const int Q = cv.P + a.G;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t b = static_cast<int64_t>(blockIdx.x) * kDeskWaves + wave;
    if (b >= a.B) return;
    const Layout y{cv.Kc, a.G, a.want_gamma != 0};
    project_inflation(a.sums + b * a.S + 1, y, cv.P, a.want_delta != 0, a.out + b * (1 + Q + static_cast<int64_t>(Q) * Q), lane,
                      kWave, [&](int k, int p) { return lj_at(cv, k, p); });
}

// -------------------------------------------------------------------------------------------------------------- host
// The waves of a block of the knot kernel: as many as the LDS budget holds (sbl::knot_waves' rule on this source's bytes),
// 0 when not even one wave's tables fit.
inline size_t block_bytes(int K, int Kc, int Pi) { return shared_bytes(K, Kc) + infl_doubles(Pi) * sizeof(double); }
inline int knot_waves(int K, int Kc, int Pi, bool gamma) {
    const size_t per_wave = static_cast<size_t>(Layout{Kc, Pi, gamma}.size()) * sizeof(double), shared = block_bytes(K, Kc, Pi);
    if (shared + per_wave > scen::kLdsBudget) return 0;
    return static_cast<int>(std::min<size_t>(kMaxWaves, (scen::kLdsBudget - shared) / per_wave));
}

inline KnotGrid knot_grid(const adr_ctx* ctx, const CurveDev& cv, int Pi, bool gamma, int64_t cap) {
    const int waves = knot_waves(cv.K, cv.Kc, Pi, gamma);
    const size_t lds = block_bytes(cv.K, cv.Kc, Pi) + static_cast<size_t>(waves) * Layout{cv.Kc, Pi, gamma}.size() * sizeof(double);
    const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(2, static_cast<int64_t>(scen::kLdsBudget / lds)));
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((cap + waves - 1) / waves, per_cu * adr_ctx_compute_units(ctx)));
    return KnotGrid{waves, lds, static_cast<unsigned>(blocks)};
}

// The scalars of an entry: the inflation scheme and pillar count, the counts, the arrays that must be there.
int check_scalars(const std::string& w, const InflCurve& ic, const Book& bk, int64_t B, const double* out) {
    if (ic.method != ADR_INTERP_FLAT_FWD_RATES && ic.method != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": inflation scheme must be FLAT_FWD_RATES (1) or LINEAR_ZERO_RATES (4)");
    if (ic.P < 1 || ic.P > ADR_YOY_MAX_PILLARS)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": the inflation curve needs 1 .. ADR_YOY_MAX_PILLARS (64) pillars");
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    if (bk.n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one swap is needed");
    if (bk.n_fix < 0 || bk.m < 0 || bk.n_fix > INT32_MAX || bk.m > INT32_MAX)
        return adr_set_error(ADR_ERR_INVALID, w + ": flow counts must lie in 0 .. 2^31 - 1");
    if (!ic.T || !ic.b) return adr_set_error(ADR_ERR_INVALID, w + ": null inflation curve arrays");
    if (!bk.fix_off || !bk.cpn_off) return adr_set_error(ADR_ERR_INVALID, w + ": null offsets (an empty leg has offsets of 0)");
    if ((bk.n_fix > 0 && (!bk.fix_tp || !bk.fix_pay)) || (bk.m > 0 && !bk.cpn))
        return adr_set_error(ADR_ERR_INVALID, w + ": null cash-flow array");
    if (!out) return adr_set_error(ADR_ERR_INVALID, w + ": out is NULL");
    return ADR_OK;
}

inline std::string fit_message(int Kc, int Pi) {
    return ": the tables of one wave (" + std::to_string(Kc) + " knots x " + std::to_string(Pi) +
           " inflation pillars) do not fit the 160 KiB LDS of a CU";
}

// The curve handle of a device entry and that the request can run on it: of this ctx, hess for GAMMA, one wave's tables in LDS.
int check_curve(const std::string& w, const adr_ctx* ctx, const adr_curve* curve, int Pi, const Request& rq, const CurveDev** cv) {
    if (!ctx || !curve) return adr_set_error(ADR_ERR_INVALID, w + ": null ctx/curve");
    const adr_ctx* owner = nullptr;
    *cv = adr_curve_device_view(curve, &owner);
    if (owner != ctx) return adr_set_error(ADR_ERR_INVALID, w + ": the curve was uploaded through another ctx");
    if (rq.gamma && !(*cv)->lc_lanes && !(*cv)->lcflat)
        return adr_set_error(ADR_ERR_INVALID, w + ": GAMMA requested but the curve was uploaded without hess");
    if (knot_waves((*cv)->K, (*cv)->Kc, Pi, rq.gamma) < 1) return adr_set_error(ADR_ERR_UNSUPPORTED, w + fit_message((*cv)->Kc, Pi));
    return ADR_OK;
}

// The host arrays of the inflation curve and of the book (yoy_scenario_pv.hip's rules and wording).
int check_host_arrays(const std::string& w, const InflCurve& ic, const Book& bk) {
    for (int k = 0; k < ic.P; ++k)
        if (!std::isfinite(ic.T[k]) || !std::isfinite(ic.b[k]) || !(ic.b[k] > -1.0) || !(ic.T[k] > (k ? ic.T[k - 1] : 0.0)))
            return adr_set_error(ADR_ERR_INVALID, w + ": pillar times must be increasing from > 0, rates finite and > -1");
    if (bk.fix_off[0] != 0 || bk.fix_off[bk.n] != bk.n_fix) return adr_set_error(ADR_ERR_INVALID, w + ": fix_off must run from 0 to the flow count");
    if (bk.cpn_off[0] != 0 || bk.cpn_off[bk.n] != bk.m) return adr_set_error(ADR_ERR_INVALID, w + ": cpn_off must run from 0 to m");
    for (int64_t i = 0; i < bk.n; ++i)
        if (bk.fix_off[i + 1] < bk.fix_off[i] || bk.cpn_off[i + 1] < bk.cpn_off[i])
            return adr_set_error(ADR_ERR_INVALID, w + ": offsets must be non-decreasing");
    for (int64_t i = 0; i < bk.n_fix; ++i)
        if (!std::isfinite(bk.fix_tp[i]) || !std::isfinite(bk.fix_pay[i]))
            return adr_set_error(ADR_ERR_INVALID, w + ": fixed-flow times and amounts must be finite");
    for (int64_t i = 0; i < ADR_YOY_FIELDS * bk.m; ++i)
        if (!std::isfinite(bk.cpn[i])) return adr_set_error(ADR_ERR_INVALID, w + ": coupon fields must be finite");
    return ADR_OK;
}

int64_t work_doubles(int Kc, int Pi, int64_t n, int64_t B, bool gamma, int64_t* chunks) {
    const int64_t cap = sub::max_chunks(n, B, kChunk);
    if (chunks) *chunks = cap;
    return (cap + B) * record_doubles(Kc, Pi, gamma);
}

// The chain on `stream`; every pointer is device memory.  work: adr_yoy_subbook_ladders_work doubles, laid out as the
// chunk records [cap][S] and the desks' sums [B][S].
int enqueue(const std::string& w, adr_ctx* ctx, const CurveDev& cv, const InflCurve& ic, const Book& bk, int64_t B, const int64_t* plan,
            const Request& rq, double* out, double* work, hipStream_t stream_or_null) {
    if (!plan) return adr_set_error(ADR_ERR_INVALID, w + ": the sub-book plan is NULL (adr_scenario_subbook_plan fills it)");
    if (!work) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_yoy_subbook_ladders_work doubles are needed)");
    hipStream_t stream = nullptr;
    const int rc = call::target_stream(w, ctx, stream_or_null, &stream);
    if (rc != ADR_OK) return rc;
    const int S = record_doubles(cv.Kc, ic.P, rq.gamma);
    const int64_t cap = sub::max_chunks(bk.n, B, kChunk);
    const sub::Plan pl = sub::plan_view(plan, B);
    double* sums = work + cap * S;                       // [B][S]
    const KnotGrid kg = knot_grid(ctx, cv, ic.P, rq.gamma, cap);
    const KnotArgs ka{cv, bk, ic, cap, pl.chunk_off + B, pl.bounds, work, S, kg.waves};
    const bool is_log = cv.method != ADR_INTERP_LINEAR_FWD_RATES;
    hipError_t e = launch_knot(rq.gamma ? (is_log ? &yoy_subbook_knot_kernel<true, true> : &yoy_subbook_knot_kernel<false, true>)
                                        : (is_log ? &yoy_subbook_knot_kernel<true, false> : &yoy_subbook_knot_kernel<false, false>),
                               ka, kg, stream);
    if (e == hipSuccess) e = sub::enqueue_sum(work, pl.chunk_off, cap, B, S, sums, stream);
    const int64_t tiles = (B + kProjDesks - 1) / kProjDesks, desk_blocks = (B + kDeskWaves - 1) / kDeskWaves;
    if (e == hipSuccess && (tiles > INT32_MAX || desk_blocks > INT32_MAX)) e = hipErrorInvalidConfiguration;
    if (e == hipSuccess) {
        const ProjectArgs pa{cv, sums, S, ic.P, B, rq.delta ? 1 : 0, rq.gamma ? 1 : 0, out};
        hipLaunchKernelGGL(yoy_project_kernel, dim3(static_cast<unsigned>(tiles), static_cast<unsigned>(cv.P + ic.P + 1)),
                           dim3(kWave * kProjWaves), 0, stream, pa);
        e = hipGetLastError();
        if (e == hipSuccess && rq.delta) {
            hipLaunchKernelGGL(yoy_infl_kernel, dim3(static_cast<unsigned>(desk_blocks)), dim3(kWave * kDeskWaves), 0, stream, pa);
            e = hipGetLastError();
        }
    }
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

// The chunks [lo, hi) of the plan on the host: work[ch] = the chunk's record.  Swap by swap, its fixed flows and then its
// coupons: the order in which adr_subbook_ladders_host walks the same flows as fixed flows of one trade.
template <bool kLog>
void host_chunks(const CurveTables& t, int method, const yoy::Infl& f, const Book& bk, const Layout& y, const int64_t* bounds, int S,
                 double* work, int64_t lo, int64_t hi) {
    const double unit[4] = {yoy::kUnitX[0], yoy::kUnitX[1], yoy::kUnitD[0], yoy::kUnitD[1]};
    for (int64_t ch = lo; ch < hi; ++ch) {
        double* rec = work + ch * S;
        std::fill(rec, rec + S, 0.0);
        const auto add = [rec](int i, double v) { rec[1 + i] = rec[1 + i] + v; };
        const scen::ChunkRange r = scen::host_chunk_range(ch, bounds, bk.n);
        for (int64_t i = r.i0; i < r.i1; ++i) {
            for (int64_t j = bk.fix_off[i]; j < bk.fix_off[i + 1]; ++j)
                add_fixed<kLog>(bk, j, t.x.data(), t.K, method, t.compact_of.data(), t.log_df.data(), y, add, rec[0]);
            for (int64_t j = bk.cpn_off[i]; j < bk.cpn_off[i + 1]; ++j)
                add_coupon<kLog>(bk, j, unit, f, t.x.data(), t.K, method, t.compact_of.data(), t.log_df.data(), y, add, rec[0]);
        }
    }
}

}  // namespace ysl
}  // namespace adr

namespace YL = adr::ysl;

extern "C" {

int64_t adr_yoy_subbook_ladders_work(const adr_curve* curve, int P_i, int64_t n, int64_t B, uint32_t req_mask, int64_t* chunks) {
    const adr_ctx* owner = nullptr;
    const adr::CurveDev* cv = adr_curve_device_view(curve, &owner);
    if (!cv || P_i < 1 || P_i > ADR_YOY_MAX_PILLARS || n < 1 || B < 1) return 0;
    return YL::work_doubles(cv->Kc, P_i, n, B, YL::request_of(req_mask).gamma, chunks);
}

int adr_yoy_subbook_ladders_dev(adr_ctx* ctx, const adr_curve* curve, int infl_method, int P_i, const double* T_dev, const double* b_dev,
                                int64_t n, int64_t n_fix, const int64_t* fix_off_dev, const double* fix_tp_dev,
                                const double* fix_pay_dev, int64_t m, const int64_t* cpn_off_dev, const double* cpn_dev, int64_t B,
                                const int64_t* plan_dev, uint32_t req_mask, double* out_dev, double* work_dev, void* stream) {
    const std::string w = "adr_yoy_subbook_ladders_dev";
    const YL::Request rq = YL::request_of(req_mask);
    const YL::InflCurve ic{infl_method, P_i, T_dev, b_dev};
    const YL::Book bk{n, n_fix, m, fix_off_dev, fix_tp_dev, fix_pay_dev, cpn_off_dev, cpn_dev};
    int rc = YL::check_scalars(w, ic, bk, B, out_dev);
    const adr::CurveDev* cv = nullptr;
    if (rc == ADR_OK) rc = YL::check_curve(w, ctx, curve, P_i, rq, &cv);
    if (rc != ADR_OK) return rc;
    return YL::enqueue(w, ctx, *cv, ic, bk, B, plan_dev, rq, out_dev, work_dev, static_cast<hipStream_t>(stream));
}

int adr_yoy_subbook_ladders(adr_ctx* ctx, const adr_curve* curve, int infl_method, int P_i, const double* T, const double* b, int64_t n,
                            int64_t n_fix, const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                            const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, uint32_t req_mask,
                            double* out) {
    const std::string w = "adr_yoy_subbook_ladders";
    const YL::Request rq = YL::request_of(req_mask);
    const YL::InflCurve ic{infl_method, P_i, T, b};
    const YL::Book bk{n, n_fix, m, fix_off, fix_tp, fix_pay, cpn_off, cpn};
    int rc = YL::check_scalars(w, ic, bk, B, out);
    const adr::CurveDev* cv = nullptr;
    if (rc == ADR_OK) rc = YL::check_curve(w, ctx, curve, P_i, rq, &cv);
    if (rc == ADR_OK) rc = YL::check_host_arrays(w, ic, bk);
    if (rc != ADR_OK) return rc;
    std::vector<int64_t> plan;
    rc = adr::sub::build_plan(w, n, B, sub_off, plan);
    if (rc != ADR_OK) return rc;
    hipStream_t stream = nullptr;
    rc = adr::call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const int Q = cv->P + P_i;
    double *dout, *dwork, *dT, *db, *dftp, *dfpay, *dcpn;
    int64_t *dplan, *dfo, *dco;
    adr::call::Staging mem;                         // `plan` is uploaded from where it stands: it outlives finish()
    mem.out(&dout, out, static_cast<size_t>(B) * (1 + Q + static_cast<size_t>(Q) * Q));
    mem.scratch(&dwork, static_cast<size_t>(YL::work_doubles(cv->Kc, P_i, n, B, rq.gamma, nullptr)));
    mem.in(&dT, T, P_i);
    mem.in(&db, b, P_i);
    mem.in(&dftp, fix_tp, n_fix);
    mem.in(&dfpay, fix_pay, n_fix);
    mem.in(&dcpn, cpn, ADR_YOY_FIELDS * static_cast<size_t>(m));
    mem.in(&dplan, plan.data(), plan.size());
    mem.in(&dfo, fix_off, n + 1);
    mem.in(&dco, cpn_off, n + 1);
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess)
        rc = YL::enqueue(w, ctx, *cv, YL::InflCurve{infl_method, P_i, dT, db}, YL::Book{n, n_fix, m, dfo, dftp, dfpay, dco, dcpn}, B,
                         dplan, rq, dout, dwork, stream);
    return mem.finish(w, rc, e, stream);
}

int adr_yoy_subbook_ladders_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac,
                                 const double* hess, int infl_method, int P_i, const double* T, const double* b, int64_t n,
                                 int64_t n_fix, const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                                 const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, uint32_t req_mask,
                                 double* out) {
    const std::string w = "adr_yoy_subbook_ladders_host";
    const YL::Request rq = YL::request_of(req_mask);
    const YL::InflCurve ic{infl_method, P_i, T, b};
    const YL::Book bk{n, n_fix, m, fix_off, fix_tp, fix_pay, cpn_off, cpn};
    int rc = YL::check_host_counts(w, interp_method, n, B);
    if (rc == ADR_OK) rc = YL::check_scalars(w, ic, bk, B, out);
    if (rc != ADR_OK) return rc;
    if (!times || !dfs || !jac) return adr_set_error(ADR_ERR_INVALID, w + ": null curve arrays");
    if (rq.gamma && !hess) return adr_set_error(ADR_ERR_INVALID, w + ": GAMMA requested but hess is NULL");
    rc = YL::check_host_arrays(w, ic, bk);
    if (rc != ADR_OK) return rc;
    std::vector<int64_t> plan;
    rc = adr::sub::build_plan(w, n, B, sub_off, plan);
    if (rc != ADR_OK) return rc;
    adr::CurveTables t;
    const std::string err = adr::build_curve_tables(K, P, times, dfs, jac, rq.gamma ? hess : nullptr, t);
    if (!err.empty()) return adr_set_error(ADR_ERR_INVALID, w + ": " + err);
    if (YL::knot_waves(t.K, t.Kc, P_i, rq.gamma) < 1) return adr_set_error(ADR_ERR_UNSUPPORTED, w + YL::fit_message(t.Kc, P_i));
    double x[adr::yoy::kNodes], L[adr::yoy::kNodes], L1[adr::yoy::kNodes], L2[adr::yoy::kNodes];
    for (int k = 0; k <= P_i; ++k) adr::yoy::make_node(T, b, k, x + k, L + k, L1 + k, L2 + k);
    const adr::yoy::Infl f{x, L, L1, L2, P_i + 1, infl_method};
    const YL::Layout y{t.Kc, P_i, rq.gamma};
    const int S = 1 + y.size(), Q = P + P_i;
    const int64_t chunks = plan[B];
    std::vector<double> work(static_cast<size_t>(chunks) * S), sums(static_cast<size_t>(B) * S);
    const int64_t* bounds = plan.data() + B + 1;
    const bool lin = interp_method == ADR_INTERP_LINEAR_FWD_RATES;
    adr::parallel_ranges(chunks, adr::pool_threads(chunks, 4), [&](int, int64_t lo, int64_t hi) {
        if (lin) YL::host_chunks<false>(t, interp_method, f, bk, y, bounds, S, work.data(), lo, hi);
        else YL::host_chunks<true>(t, interp_method, f, bk, y, bounds, S, work.data(), lo, hi);
    });
    adr::sub::reduce_subbooks(work.data(), plan.data(), B, S, sums.data());
    const size_t stride = 1 + Q + static_cast<size_t>(Q) * Q;
    adr::parallel_ranges(B, adr::pool_threads(B, 1), [&](int, int64_t lo, int64_t hi) {
        for (int64_t d = lo; d < hi; ++d) {
            const double* rec = sums.data() + d * S;
            YL::host_project_curve(t, rq, rec, Q, out + d * stride);
            YL::project_inflation(rec + 1, y, P, rq.delta, out + d * stride, 0, 1, [&](int k, int p) { return YL::host_lj(t, k, p); });
        }
    });
    return ADR_OK;
}

}  // extern "C"
