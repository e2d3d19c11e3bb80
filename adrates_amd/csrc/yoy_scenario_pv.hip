// Inflation scenario revaluation: the PV of every YoY inflation swap of a book under S scenarios, each a pair of a
// discount curve row and a breakeven row (adr_yoy_scenario_pv*; declarations, semantics and the order of the book sum:
// include/adrates.h).
//
// pv[i][s] = sum_f fix_pay_f D_s(tp_f) [tp_f > 0] + sum_j scale_j (I_s(te_j) / I_s(ts_j) - 1 + spread_j) D_s(tp_j) [tp_j > 0]:
// D_s is InterpolatorAd.simple_interpolate on (times, dfs[s]) exactly as scenario_pv.hip reads it, I_s the same rule on
// the nodes (0, 1), (T_k, (1 + b[s][k])^T_k) as yoy_risk.hip forms them.  Both inflation schemes make ln I(t) a weighted
// sum of at most two L_k = T_k ln(1 + b_k) (simple_interp.hpp::log_weights), so a YoY ratio is ONE exp of the
// difference of two such sums.
//
// Layout, lookup form, lane broadcast and book sum: scenario_common.hpp, swaps for trades.  Beside the group's discount
// table the block holds the group's inflation table itab[k][lane] = L_k.  Where the two do not fit together the small
// inflation table stays in LDS and the lanes read their discount rows from global memory.  Lane l describes index l of
// the swap - YoY coupon l and fixed flow l: their segment searches, knot indices and weights - and marks what needs no
// evaluation of its own: a YoY start equal to the previous coupon's end (annual legs tile: the weighted sum is the one
// just computed), ts == te (y = 0 exactly), a fixed flow paid with the coupon of the same index (one D(tp) for both).
// The wave then walks the indices in order, fetching index j's description from lane j with v_readlane into scalar
// registers, and each lane evaluates on its own scenario's tables.
//
// A shared curve (S_disc = 1 or S_infl = 1: "not shocked") is read with row stride 0.  The host twin
// (adr_yoy_scenario_pv_host) runs the same per-date and per-coupon code in the same order on CPU threads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "host_pool.hpp"
#include "scenario_common.hpp"
#include "subbook.hpp"

#pragma clang fp contract(off)      // as scenario_common.hpp: the host and the device evaluate the same expressions

namespace adr {
namespace yscen {

using namespace scen;    // the shared pieces (scenario_common.hpp)

// A date on the inflation table (Tb_k = L_k, L_0 = 0) has scenario_common.hpp's weight form too:
//   ln I = (a > 0 ? wa L_a : 0) + (b != a ? wb L_b : 0).
__host__ __device__ inline DateW infl_weights(double t, const double* x, int N, int method) {
    const si::LogWeights w = si::log_weights(t, x, N, method);
    return DateW{w.a, w.b, w.wa, w.wb};
}

template <class Tab>
__host__ __device__ inline double eval_ln_index(const DateW& d, const Tab& itab) {
    double s = 0.0;
    if (d.a > 0) s = d.wa * itab(d.a);          // knot 0 is (0, 1): L = 0 whatever its weight
    if (d.b != d.a) s = s + d.wb * itab(d.b);
    return s;
}

// L_k of a breakeven row, as yoy_risk.hip::make_node forms it (k >= 1; L_0 = 0).
__host__ __device__ inline double node_log(const double* T, const double* b, int k) {
    if (k == 0) return 0.0;
    const double ob = 1.0 + b[k - 1];
    return T[k - 1] * log(ob);
}

// Index c of a swap: its YoY coupon (c < n_cpn) and its fixed flow (c < n_fix).  Both masks are strict (tp > 0).
enum : int {
    kHasCpn = 1, kHasFix = 2,
    kTsIsPrevTe = 4,     // YoY start == the previous coupon's YoY end: ln I(ts) is the ln I(te) just computed
    kTsIsTe = 8,         // y = 0 exactly: no lookups, no exp
    kFixIsCpnTp = 16     // the fixed flow is paid with the coupon: D is D(tp)
};

struct Slot {
    int flags;
    DateW wp, wx, ws, we;       // D(tp) of the coupon, D of the fixed flow, ln I(ts), ln I(te)
    double scale, spread, pay;
};

__host__ __device__ inline Slot empty_slot() {
    Slot s;
    s.flags = 0;
    s.wp = s.wx = s.ws = s.we = DateW{0, 0, 0.0, 0.0};
    s.scale = 0.0; s.spread = 0.0; s.pay = 0.0;
    return s;
}

struct Legs {            // one swap's cash flows
    const double *fix_tp, *fix_pay, *cpn;
    int64_t m, f0, c0;
    int n_fix, n_cpn;
};

struct Curves {          // what a description needs of the curves: the knots, not the values
    const double *x, *ix;
    int K, N, dm, im;    // N = P + 1 inflation nodes
};

template <bool kLog>
__host__ __device__ inline Slot make_slot(const Legs& g, int c, const Curves& cv) {
    Slot s = empty_slot();
    double tp = 0.0;
    bool cpn = false;
    if (c < g.n_cpn) {
        tp = g.cpn[ADR_YOY_TP * g.m + g.c0 + c];
        cpn = tp > 0.0;
    }
    if (cpn) {
        const int64_t i = g.c0 + c;
        const double ts = g.cpn[ADR_YOY_TS * g.m + i], te = g.cpn[ADR_YOY_TE * g.m + i];
        s.flags |= kHasCpn;
        s.scale = g.cpn[ADR_YOY_SCALE * g.m + i];
        s.spread = g.cpn[ADR_YOY_SPREAD * g.m + i];
        if (ts == te) {
            s.flags |= kTsIsTe;
        } else {
            // the previous coupon left its ln I(te) behind when it counted and looked it up
            bool prev = false;
            if (c > 0) {
                const double pte = g.cpn[ADR_YOY_TE * g.m + i - 1];
                prev = ts == pte && g.cpn[ADR_YOY_TP * g.m + i - 1] > 0.0 && g.cpn[ADR_YOY_TS * g.m + i - 1] != pte;
            }
            if (prev) s.flags |= kTsIsPrevTe;
            else s.ws = infl_weights(ts, cv.ix, cv.N, cv.im);
            s.we = infl_weights(te, cv.ix, cv.N, cv.im);
        }
        s.wp = date_weights<kLog>(tp, cv.x, cv.K, cv.dm);
    }
    if (c < g.n_fix) {
        const double xt = g.fix_tp[g.f0 + c];
        if (xt > 0.0) {
            s.flags |= kHasFix;
            s.pay = g.fix_pay[g.f0 + c];
            if (cpn && xt == tp) s.flags |= kFixIsCpnTp;
            else s.wx = date_weights<kLog>(xt, cv.x, cv.K, cv.dm);
        }
    }
    return s;
}

struct Acc {             // one scenario's running state inside a swap
    double le, cpn, fix; // ln I(te) of the previous coupon; the legs' sums
};

template <bool kLog, class Tab, class ITab>
__host__ __device__ inline void apply_slot(const Slot& s, const Tab& tab, const ITab& itab, Acc& a) {
    double dp = 0.0;
    if (s.flags & kHasCpn) {
        dp = eval_df<kLog>(s.wp, tab);
        double y = 0.0;
        if (!(s.flags & kTsIsTe)) {
            const double ls = (s.flags & kTsIsPrevTe) ? a.le : eval_ln_index(s.ws, itab);
            const double le = eval_ln_index(s.we, itab);
            y = exp(le - ls) - 1.0;
            a.le = le;
        }
        a.cpn = a.cpn + (s.scale * (y + s.spread)) * dp;
    }
    if (s.flags & kHasFix) {
        const double dx = (s.flags & kFixIsCpnTp) ? dp : eval_df<kLog>(s.wx, tab);
        a.fix = a.fix + s.pay * dx;
    }
}

__host__ __device__ inline double swap_pv(const Acc& a) { return a.fix + a.cpn; }

// A leg's range of swap i, or false when the offsets cannot be right (then nothing of the leg is read).
__host__ __device__ inline bool leg_range(const int64_t* off, int64_t i, int64_t total, int64_t* begin, int* count) {
    const int64_t lo = off[i], hi = off[i + 1];
    if (lo < 0 || hi < lo || hi > total || hi - lo > INT32_MAX) return false;
    *begin = lo;
    *count = static_cast<int>(hi - lo);
    return true;
}

// ------------------------------------------------------------------------------------------------------------ device
struct Args {
    const double *times, *dfs;       // [K], [S_disc][K]
    const double *T, *b;             // [P], [S_infl][P]
    int K, P, S, dm, im;
    int disc_stride, infl_stride;    // K / P, or 0 for a shared row
    int64_t n, mf, m;
    int64_t n_chunks;                // kSub: the rows `work` holds, an upper bound of the plan's count
    const int64_t *fix_off, *cpn_off;
    const double *fix_tp, *fix_pay, *cpn;
    double *pv, *work;               // [n][S] or null; [n_chunks][S]
    const int64_t *sub_chunks, *sub_bounds;      // kSub: the plan's chunk count and its [chunks][2] swap bounds (subbook.hpp)
};

// Lane j's slot in scalar registers; only the parts its flags say will be read.
__device__ inline Slot lane_slot(const Slot& m, int j) {
    Slot u = empty_slot();
    u.flags = lane_int(m.flags, j);
    if (u.flags & kHasCpn) {
        u.wp = lane_date(m.wp, j);
        if (!(u.flags & kTsIsTe)) {
            if (!(u.flags & kTsIsPrevTe)) u.ws = lane_date(m.ws, j);
            u.we = lane_date(m.we, j);
        }
        u.scale = lane_dbl(m.scale, j);
        u.spread = lane_dbl(m.spread, j);
    }
    if (u.flags & kHasFix) {
        if (!(u.flags & kFixIsCpnTp)) u.wx = lane_date(m.wx, j);
        u.pay = lane_dbl(m.pay, j);
    }
    return u;
}

struct DevITab {
    const double* p;     // &itab[0][lane]
    __device__ double operator()(int k) const { return p[k * kWave]; }
};

// kSub: the chunks are those of a sub-book plan (their swap bounds come from a table) instead of ch * kChunk.
template <bool kLog, bool kLds, bool kSub>
__global__ __launch_bounds__(kThreads) void yoy_scenario_pv_kernel(Args a) {
    extern __shared__ double lds[];
    const int K = a.K, N = a.P + 1, S = a.S;
    double* s_x = lds;                               // [K]
    double* s_ix = s_x + K;                          // [N]
    double* s_itab = s_ix + N;                       // [N][64]
    double* s_tab = s_itab + N * kWave;              // [K][64] (kLds)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t s = static_cast<int64_t>(blockIdx.y) * kWave + lane;
    const bool live = s < S;
    const int64_t sr = live ? s : S - 1;                    // padding lanes price the last scenario and store nothing
    const double* row = a.dfs + sr * a.disc_stride;
    const double* brow = a.b + sr * a.infl_stride;
    for (int k = threadIdx.x; k < K; k += kThreads) s_x[k] = a.times[k];
    for (int k = threadIdx.x; k < N; k += kThreads) s_ix[k] = k ? a.T[k - 1] : 0.0;
    for (int k = wave; k < N; k += kWaves) s_itab[k * kWave + lane] = node_log(a.T, brow, k);
    if (kLds)
        for (int k = wave; k < K; k += kWaves) s_tab[k * kWave + lane] = kLog ? log(row[k]) : row[k];
    __syncthreads();
    const DevTab<kLog, kLds> tab{kLds ? s_tab + lane : row};
    const DevITab itab{s_itab + lane};
    const Curves cv{s_x, s_ix, K, N, a.dm, a.im};
    int64_t n_chunks = a.n_chunks;
    if (kSub) {
        const int64_t planned = *a.sub_chunks;              // uniform: a scalar load
        n_chunks = planned < n_chunks ? planned : n_chunks;
    }
    for (int64_t ch = static_cast<int64_t>(blockIdx.x) * kWaves + wave; ch < n_chunks;
         ch += static_cast<int64_t>(gridDim.x) * kWaves) {
        const ChunkRange r = chunk_range<kSub>(ch, a.sub_bounds, a.n);
        double book = 0.0;
        for (int64_t i = r.i0; i < r.i1; ++i) {
            Legs g{a.fix_tp, a.fix_pay, a.cpn, a.m, 0, 0, 0, 0};      // uniform: scalar loads
            const bool ok_fix = leg_range(a.fix_off, i, a.mf, &g.f0, &g.n_fix);
            const bool ok = leg_range(a.cpn_off, i, a.m, &g.c0, &g.n_cpn) && ok_fix;
            const int cnt_all = ok ? (g.n_fix > g.n_cpn ? g.n_fix : g.n_cpn) : 0;
            Acc acc{0.0, 0.0, 0.0};
            for (int base = 0; base < cnt_all; base += kWave) {
                const int cnt = cnt_all - base < kWave ? cnt_all - base : kWave;
                Slot mine = empty_slot();
                if (lane < cnt) mine = make_slot<kLog>(g, base + lane, cv);
                for (int j = 0; j < cnt; ++j) apply_slot<kLog>(lane_slot(mine, j), tab, itab, acc);
            }
            const double pv = ok ? swap_pv(acc) : NAN;             // malformed offsets: no reads, a NaN PV
            if (a.pv && live) a.pv[i * S + s] = pv;
            book = book + pv;
        }
        if (live) a.work[ch * S + s] = book;
    }
}

// -------------------------------------------------------------------------------------------------------------- host
inline size_t lds_bytes(int K, int P, bool table) {
    const size_t N = static_cast<size_t>(P) + 1;
    return (static_cast<size_t>(K) + N + N * kWave + (table ? static_cast<size_t>(K) * kWave : 0)) * sizeof(double);
}

struct Call {            // the scalars and pointers of one call, host or device
    int dm, K;
    const double* times;
    int S_disc;
    const double* dfs;
    int im, P;
    const double* T;
    int S_infl;
    const double* b;
    int S;
    int64_t n, mf;
    const int64_t* fix_off;
    const double *fix_tp, *fix_pay;
    int64_t m;
    const int64_t* cpn_off;
    const double* cpn;
    double *pv, *book;
};

int validate(const std::string& w, const Call& c) {
    if (c.dm != ADR_INTERP_FLAT_FWD_RATES && c.dm != ADR_INTERP_LINEAR_FWD_RATES && c.dm != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": discount scheme must be FLAT_FWD_RATES (1), LINEAR_FWD_RATES (2) or "
                                                      "LINEAR_ZERO_RATES (4)");
    if (c.im != ADR_INTERP_FLAT_FWD_RATES && c.im != ADR_INTERP_LINEAR_ZERO_RATES)
        return adr_set_error(ADR_ERR_UNSUPPORTED, w + ": inflation scheme must be FLAT_FWD_RATES (1) or LINEAR_ZERO_RATES (4)");
    if (c.K < 2 || c.K > ADR_SCENARIO_MAX_KNOTS)
        return adr_set_error(ADR_ERR_INVALID, w + ": the knot grid needs 2 .. ADR_SCENARIO_MAX_KNOTS (4096) knots");
    if (c.P < 1 || c.P > ADR_YOY_MAX_PILLARS)
        return adr_set_error(ADR_ERR_INVALID, w + ": the inflation curve needs 1 .. ADR_YOY_MAX_PILLARS (64) pillars");
    if (c.S < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one scenario is needed");
    if ((c.S_disc != 1 && c.S_disc != c.S) || (c.S_infl != 1 && c.S_infl != c.S))
        return adr_set_error(ADR_ERR_INVALID, w + ": S_disc and S_infl must each be 1 (a shared curve) or S");
    if (c.n < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one swap is needed");
    if (c.mf < 0 || c.m < 0 || c.mf > INT32_MAX || c.m > INT32_MAX)
        return adr_set_error(ADR_ERR_INVALID, w + ": flow counts must lie in 0 .. 2^31 - 1");
    if (!c.times || !c.dfs || !c.T || !c.b) return adr_set_error(ADR_ERR_INVALID, w + ": null curve arrays");
    if (!c.fix_off || !c.cpn_off) return adr_set_error(ADR_ERR_INVALID, w + ": null offsets (an empty leg has offsets of 0)");
    if ((c.mf > 0 && (!c.fix_tp || !c.fix_pay)) || (c.m > 0 && !c.cpn))
        return adr_set_error(ADR_ERR_INVALID, w + ": null cash-flow array");
    if (!c.book) return adr_set_error(ADR_ERR_INVALID, w + ": book_pv is NULL");
    return ADR_OK;
}

int check_host_arrays(const std::string& w, const Call& c) {
    const int rc = check_curves(w, c.K, c.times, c.S_disc, c.dfs, "row");
    if (rc != ADR_OK) return rc;
    for (int k = 0; k < c.P; ++k)
        if (!std::isfinite(c.T[k]) || !(c.T[k] > (k ? c.T[k - 1] : 0.0)))
            return adr_set_error(ADR_ERR_INVALID, w + ": pillar times must be increasing from > 0");
    for (int64_t i = 0; i < static_cast<int64_t>(c.S_infl) * c.P; ++i)
        if (!std::isfinite(c.b[i]) || !(c.b[i] > -1.0))
            return adr_set_error(ADR_ERR_INVALID, w + ": breakeven rates must be finite and > -1 (row " +
                                                      std::to_string(i / c.P) + ", pillar " + std::to_string(i % c.P) + ")");
    if (c.fix_off[0] != 0 || c.fix_off[c.n] != c.mf) return adr_set_error(ADR_ERR_INVALID, w + ": fix_off must run from 0 to the flow count");
    if (c.cpn_off[0] != 0 || c.cpn_off[c.n] != c.m) return adr_set_error(ADR_ERR_INVALID, w + ": cpn_off must run from 0 to m");
    for (int64_t i = 0; i < c.n; ++i)
        if (c.fix_off[i + 1] < c.fix_off[i] || c.cpn_off[i + 1] < c.cpn_off[i])
            return adr_set_error(ADR_ERR_INVALID, w + ": offsets must be non-decreasing");
    for (int64_t i = 0; i < c.mf; ++i)
        if (!std::isfinite(c.fix_tp[i]) || !std::isfinite(c.fix_pay[i]))
            return adr_set_error(ADR_ERR_INVALID, w + ": fixed-flow times and amounts must be finite");
    for (int64_t i = 0; i < ADR_YOY_FIELDS * c.m; ++i)
        if (!std::isfinite(c.cpn[i])) return adr_set_error(ADR_ERR_INVALID, w + ": coupon fields must be finite");
    return ADR_OK;
}

template <bool kLog, bool kLds>
hipError_t launch(const Args& a, dim3 grid, hipStream_t stream) {
    const size_t lds = lds_bytes(a.K, a.P, kLds);
    if (a.sub_bounds) return launch_with_lds(&yoy_scenario_pv_kernel<kLog, kLds, true>, a, lds, grid, stream);
    return launch_with_lds(&yoy_scenario_pv_kernel<kLog, kLds, false>, a, lds, grid, stream);
}

// The two kernels on `stream`; every pointer of `c` is device memory.  B > 0: the chunks of the sub-book plan `plan`, and
// c.book is sub_pv[B][S].
int enqueue(const std::string& w, adr_ctx* ctx, const Call& c, double* work, hipStream_t stream_or_null, int64_t B = 0,
            const int64_t* plan = nullptr) {
    int rc = validate(w, c);
    if (rc != ADR_OK) return rc;
    if (!work) return adr_set_error(ADR_ERR_INVALID, w + ": work is NULL (adr_yoy_scenario_pv_work doubles are needed)");
    const bool subs = B != 0 || plan;
    if (subs && B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    if (subs && !plan) return adr_set_error(ADR_ERR_INVALID, w + ": the sub-book plan is NULL (adr_scenario_subbook_plan fills it)");
    hipStream_t stream = nullptr;
    rc = call::target_stream(w, ctx, stream_or_null, &stream);
    if (rc != ADR_OK) return rc;
    const int64_t chunks = subs ? sub::max_chunks(c.n, B, kChunk) : (c.n + kChunk - 1) / kChunk;
    dim3 grid;
    rc = launch_grid(w, ctx, chunks, c.S, &grid);
    if (rc != ADR_OK) return rc;
    const sub::Plan pl = subs ? sub::plan_view(plan, B) : sub::Plan{nullptr, nullptr};
    const Args a{c.times, c.dfs, c.T, c.b, c.K, c.P, c.S, c.dm, c.im, c.S_disc == 1 ? 0 : c.K, c.S_infl == 1 ? 0 : c.P,
                 c.n, c.mf, c.m, chunks, c.fix_off, c.cpn_off, c.fix_tp, c.fix_pay, c.cpn, c.pv, work,
                 subs ? pl.chunk_off + B : nullptr, pl.bounds};
    const bool in_lds = lds_bytes(c.K, c.P, true) <= kLdsBudget;
    const bool lin = c.dm == ADR_INTERP_LINEAR_FWD_RATES;
    hipError_t e;
    if (lin) e = in_lds ? launch<false, true>(a, grid, stream) : launch<false, false>(a, grid, stream);
    else e = in_lds ? launch<true, true>(a, grid, stream) : launch<true, false>(a, grid, stream);
    if (e == hipSuccess && subs) e = sub::enqueue_sum(work, pl.chunk_off, chunks, B, c.S, c.book, stream);
    else if (e == hipSuccess) e = enqueue_book_sum(work, chunks, c.S, c.book, stream);
    if (e != hipSuccess) return adr_set_error(ADR_ERR_HIP, w + ": " + hipGetErrorString(e));
    return ADR_OK;
}

template <bool kLog>
void host_chunks(const Call& c, const Curves& cv, const double* tab, const double* itab, double* work, int64_t lo, int64_t hi,
                 const int64_t* bounds = nullptr) {
    const int S = c.S, N = c.P + 1;
    const size_t ds = c.S_disc == 1 ? 0 : c.K, is = c.S_infl == 1 ? 0 : N;
    std::vector<Acc> acc(static_cast<size_t>(S));
    std::vector<double> book(static_cast<size_t>(S));
    for (int64_t ch = lo; ch < hi; ++ch) {
        std::fill(book.begin(), book.end(), 0.0);
        const ChunkRange r = host_chunk_range(ch, bounds, c.n);
        for (int64_t i = r.i0; i < r.i1; ++i) {
            Legs g{c.fix_tp, c.fix_pay, c.cpn, c.m, 0, 0, 0, 0};
            const bool ok_fix = leg_range(c.fix_off, i, c.mf, &g.f0, &g.n_fix);
            const bool ok = leg_range(c.cpn_off, i, c.m, &g.c0, &g.n_cpn) && ok_fix;
            std::fill(acc.begin(), acc.end(), Acc{0.0, 0.0, 0.0});
            for (int j = 0; ok && j < std::max(g.n_fix, g.n_cpn); ++j) {
                const Slot slot = make_slot<kLog>(g, j, cv);
                for (int s = 0; s < S; ++s)
                    apply_slot<kLog>(slot, HostTab{tab + static_cast<size_t>(s) * ds}, HostTab{itab + static_cast<size_t>(s) * is}, acc[s]);
            }
            for (int s = 0; s < S; ++s) {
                const double v = ok ? swap_pv(acc[s]) : NAN;
                if (c.pv) c.pv[i * S + s] = v;
                book[s] = book[s] + v;
            }
        }
        std::copy(book.begin(), book.end(), work + ch * S);
    }
}

// Blocking form: inputs, outputs and scratch in one device allocation.  B > 0: h.book is sub_pv[B][S] of the sub-books
// sub_off (host), and the plan is built and uploaded here.
int run_blocking(const std::string& w, adr_ctx* ctx, const Call& h, int64_t B = 0, const int64_t* sub_off = nullptr) {
    int rc = validate(w, h);
    if (rc == ADR_OK) rc = check_host_arrays(w, h);
    if (rc != ADR_OK) return rc;
    std::vector<int64_t> plan;
    if (B > 0) {
        rc = sub::build_plan(w, h.n, B, sub_off, plan);
        if (rc != ADR_OK) return rc;
    }
    hipStream_t stream = nullptr;
    rc = call::target_stream(w, ctx, nullptr, &stream);
    if (rc != ADR_OK) return rc;
    const int K = h.K, P = h.P, S = h.S;
    const int64_t n = h.n;
    const size_t rows = B > 0 ? static_cast<size_t>(B) : 1;
    double *dt, *ddf, *dT, *db, *dftp, *dfpay, *dcpn, *dpv, *dbook, *dwork;
    int64_t *dplan, *dfo, *dco;
    call::Staging mem;                              // `plan` is uploaded from where it stands: it outlives finish()
    mem.in(&dt, h.times, K);
    mem.in(&ddf, h.dfs, static_cast<size_t>(h.S_disc) * K);
    mem.in(&dT, h.T, P);
    mem.in(&db, h.b, static_cast<size_t>(h.S_infl) * P);
    mem.in(&dftp, h.fix_tp, h.mf);
    mem.in(&dfpay, h.fix_pay, h.mf);
    mem.in(&dcpn, h.cpn, ADR_YOY_FIELDS * static_cast<size_t>(h.m));
    mem.in(&dplan, plan.data(), plan.size());
    mem.in(&dfo, h.fix_off, n + 1);
    mem.in(&dco, h.cpn_off, n + 1);
    mem.out(&dpv, h.pv, static_cast<size_t>(n) * S, h.pv != nullptr);
    mem.out(&dbook, h.book, rows * S);
    mem.scratch(&dwork, static_cast<size_t>(B > 0 ? adr_scenario_subbook_work(n, B, S) : adr_yoy_scenario_pv_work(n, S)));
    const hipError_t e = mem.begin(stream);
    if (e == hipSuccess) {
        const Call c{h.dm, K, dt, h.S_disc, ddf, h.im, P, dT, h.S_infl, db, S, n, h.mf, dfo, dftp, dfpay, h.m, dco, dcpn, dpv, dbook};
        rc = enqueue(w, ctx, c, dwork, stream, B, dplan);
    }
    return mem.finish(w, rc, e, stream);
}

// The host entries' body; B > 0: c.book is sub_pv[B][S] of the sub-books sub_off.
int host_run(const std::string& w, const Call& c, int n_threads, int64_t B = 0, const int64_t* sub_off = nullptr) {
    int rc = validate(w, c);
    if (rc == ADR_OK) rc = check_host_arrays(w, c);
    if (rc != ADR_OK) return rc;
    std::vector<int64_t> plan;
    if (B > 0) {
        rc = sub::build_plan(w, c.n, B, sub_off, plan);
        if (rc != ADR_OK) return rc;
    }
    const bool lin = c.dm == ADR_INTERP_LINEAR_FWD_RATES;
    const int N = c.P + 1, S = c.S;
    std::vector<double> tab(c.dfs, c.dfs + static_cast<size_t>(c.S_disc) * c.K);
    if (!lin)
        for (double& v : tab) v = std::log(v);
    std::vector<double> ix(N), itab(static_cast<size_t>(c.S_infl) * N);
    for (int k = 0; k < N; ++k) ix[k] = k ? c.T[k - 1] : 0.0;
    for (int s = 0; s < c.S_infl; ++s)
        for (int k = 0; k < N; ++k) itab[static_cast<size_t>(s) * N + k] = node_log(c.T, c.b + static_cast<size_t>(s) * c.P, k);
    const Curves cv{c.times, ix.data(), c.K, N, c.dm, c.im};
    const int64_t* bounds = B > 0 ? plan.data() + B + 1 : nullptr;
    const int64_t chunks = B > 0 ? plan[B] : (c.n + kChunk - 1) / kChunk;
    std::vector<double> work(static_cast<size_t>(chunks) * S);
    const int threads = n_threads > 0 ? static_cast<int>(std::min<int64_t>(n_threads, chunks)) : adr::pool_threads(chunks, 4);
    adr::parallel_ranges(chunks, threads, [&](int, int64_t lo, int64_t hi) {
        if (lin) host_chunks<false>(c, cv, tab.data(), itab.data(), work.data(), lo, hi, bounds);
        else host_chunks<true>(c, cv, tab.data(), itab.data(), work.data(), lo, hi, bounds);
    });
    if (B > 0) sub::reduce_subbooks(work.data(), plan.data(), B, S, c.book);
    else reduce_chunks(work.data(), chunks, S, c.book);
    return ADR_OK;
}

}  // namespace yscen
}  // namespace adr

namespace YS = adr::yscen;

extern "C" {

int64_t adr_yoy_scenario_pv_work(int64_t n, int S) { return adr_scenario_pv_work(n, S); }     // the same chunks

int adr_yoy_scenario_pv_dev(adr_ctx* ctx, int disc_method, int K, const double* times_dev, int S_disc, const double* dfs_dev,
                            int infl_method, int P, const double* T_dev, int S_infl, const double* b_dev, int S, int64_t n,
                            int64_t n_fix, const int64_t* fix_off_dev, const double* fix_tp_dev, const double* fix_pay_dev,
                            int64_t m, const int64_t* cpn_off_dev, const double* cpn_dev, double* pv_dev, double* book_pv_dev,
                            double* work_dev, void* stream) {
    const YS::Call c{disc_method, K, times_dev, S_disc, dfs_dev, infl_method, P, T_dev, S_infl, b_dev, S, n, n_fix,
                     fix_off_dev, fix_tp_dev, fix_pay_dev, m, cpn_off_dev, cpn_dev, pv_dev, book_pv_dev};
    return YS::enqueue("adr_yoy_scenario_pv_dev", ctx, c, work_dev, static_cast<hipStream_t>(stream));
}

int adr_yoy_scenario_pv(adr_ctx* ctx, int disc_method, int K, const double* times, int S_disc, const double* dfs,
                        int infl_method, int P, const double* T, int S_infl, const double* b, int S, int64_t n, int64_t n_fix,
                        const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m, const int64_t* cpn_off,
                        const double* cpn, double* pv, double* book_pv) {
    const YS::Call h{disc_method, K, times, S_disc, dfs, infl_method, P, T, S_infl, b, S, n, n_fix,
                     fix_off, fix_tp, fix_pay, m, cpn_off, cpn, pv, book_pv};
    return YS::run_blocking("adr_yoy_scenario_pv", ctx, h);
}

int adr_yoy_scenario_pv_host(int disc_method, int K, const double* times, int S_disc, const double* dfs, int infl_method,
                             int P, const double* T, int S_infl, const double* b, int S, int64_t n, int64_t n_fix,
                             const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                             const int64_t* cpn_off, const double* cpn, double* pv, double* book_pv, int n_threads) {
    const YS::Call c{disc_method, K, times, S_disc, dfs, infl_method, P, T, S_infl, b, S, n, n_fix,
                     fix_off, fix_tp, fix_pay, m, cpn_off, cpn, pv, book_pv};
    return YS::host_run("adr_yoy_scenario_pv_host", c, n_threads);
}

int adr_yoy_scenario_subbook_pv(adr_ctx* ctx, int disc_method, int K, const double* times, int S_disc, const double* dfs,
                                int infl_method, int P, const double* T, int S_infl, const double* b, int S, int64_t n,
                                int64_t n_fix, const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                                const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, double* pv,
                                double* sub_pv) {
    const std::string w = "adr_yoy_scenario_subbook_pv";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const YS::Call h{disc_method, K, times, S_disc, dfs, infl_method, P, T, S_infl, b, S, n, n_fix,
                     fix_off, fix_tp, fix_pay, m, cpn_off, cpn, pv, sub_pv};
    return YS::run_blocking(w, ctx, h, B, sub_off);
}

int adr_yoy_scenario_subbook_pv_dev(adr_ctx* ctx, int disc_method, int K, const double* times_dev, int S_disc,
                                    const double* dfs_dev, int infl_method, int P, const double* T_dev, int S_infl,
                                    const double* b_dev, int S, int64_t n, int64_t n_fix, const int64_t* fix_off_dev,
                                    const double* fix_tp_dev, const double* fix_pay_dev, int64_t m, const int64_t* cpn_off_dev,
                                    const double* cpn_dev, int64_t B, const int64_t* plan_dev, double* pv_dev, double* sub_pv_dev,
                                    double* work_dev, void* stream) {
    const std::string w = "adr_yoy_scenario_subbook_pv_dev";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const YS::Call c{disc_method, K, times_dev, S_disc, dfs_dev, infl_method, P, T_dev, S_infl, b_dev, S, n, n_fix,
                     fix_off_dev, fix_tp_dev, fix_pay_dev, m, cpn_off_dev, cpn_dev, pv_dev, sub_pv_dev};
    return YS::enqueue(w, ctx, c, work_dev, static_cast<hipStream_t>(stream), B, plan_dev);
}

int adr_yoy_scenario_subbook_pv_host(int disc_method, int K, const double* times, int S_disc, const double* dfs, int infl_method,
                                     int P, const double* T, int S_infl, const double* b, int S, int64_t n, int64_t n_fix,
                                     const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                                     const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, double* pv,
                                     double* sub_pv, int n_threads) {
    const std::string w = "adr_yoy_scenario_subbook_pv_host";
    if (B < 1) return adr_set_error(ADR_ERR_INVALID, w + ": at least one sub-book is needed");
    const YS::Call c{disc_method, K, times, S_disc, dfs, infl_method, P, T, S_infl, b, S, n, n_fix,
                     fix_off, fix_tp, fix_pay, m, cpn_off, cpn, pv, sub_pv};
    return YS::host_run(w, c, n_threads, B, sub_off);
}

}  // extern "C"
