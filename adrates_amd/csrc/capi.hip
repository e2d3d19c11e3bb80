// C-ABI of libadrates_hip.so (declarations and reference citations: include/adrates.h).
#include <hip/hip_runtime.h>
#include <cmath>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/adrates.h"
#include "curve_tables.hpp"
#include "device_owner.hpp"
#include "host_pool.hpp"
#include "kernels.hpp"
#include "route.hpp"
#include "schedule_groups.hpp"

namespace {

thread_local std::string g_last_error;

constexpr size_t kLdsBudget = 160 * 1024;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int fail_hip(hipError_t e, const char* what) {
    return fail(ADR_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define ADR_HIP(call)                                      \
    do {                                                   \
        hipError_t e__ = (call);                           \
        if (e__ != hipSuccess) return fail_hip(e__, #call); \
    } while (0)

// The interpolation schemes the kernels implement; `who`: the entry point, for the message.
int check_interp(int method, const char* who) {
    if (method == ADR_INTERP_FLAT_FWD_RATES || method == ADR_INTERP_LINEAR_ZERO_RATES || method == ADR_INTERP_LINEAR_FWD_RATES)
        return ADR_OK;
    return fail(ADR_ERR_UNSUPPORTED, std::string(who) + ": only FLAT_FWD_RATES (1), LINEAR_FWD_RATES (2) and "
                                                        "LINEAR_ZERO_RATES (4) are implemented");
}

// Every array of a batch and of its schedule groups has this much room behind it: the kernels' neighbour reads (a header's
// worth past the last element) never leave the buffer.  The curve arrays have none: the kernels read them by table sizes.
constexpr size_t kBatchPad = 64;

}  // namespace

struct adr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    int n_cu = 0;
    size_t lds_limit = 0;
    double* partials = nullptr;     // [max_blocks][kAggStride] scratch for the aggregate
    double* dump = nullptr;                 // [32*32] store sink (kernels.hpp, OutputsDev::dump)
    unsigned long long* stamps = nullptr;   // diagnostic builds: [max_blocks*16][8]
    int max_blocks = 0;
    // aggregate-only mode (kernels_knot.hip): block records [knot_blocks][1 + 3 Kc] of the knot-space kernel and their sum
    double* knot_partials = nullptr;
    double* knot_reduced = nullptr;
    double* knot_overflow = nullptr;        // [kKnotLagMaxKc^2] pairs of knots beyond the bands (payment-lag rows)
    int knot_blocks = 0;
};

namespace {
namespace R = adr::route;
constexpr int kKnotStrideMax = std::max(1 + 3 * R::kKnotMaxKc, 1 + (2 + adr::kKnotBand) * R::kKnotLagMaxKc);

// The structural half of a curve's device image - everything that follows from the knot grid and the sparsity of the
// Jacobians, not from the curve's values: uploads those tables into `mem` and sets every such field of `c`.  An uploaded
// curve (adr_curve_upload_ex) adds its value arrays, a curve plan (adr_curve_plan_create) shares this half among the curves
// built from it, so a field set here is set for both.  `wide`: the wide layout's index tables are wanted (the callers decide
// differently).  Returns with its copies done (they read vectors of this function); errors are left in `mem`.
void fill_curve_structure(const adr::CurveTables& t, int method, const R::CurveClass& cls, bool wide, adr::DeviceOwner& mem,
                          hipStream_t stream, adr::CurveDev& c) {
    const std::vector<int16_t> first16(t.first_of.begin(), t.first_of.end()), comp16(t.compact_of.begin(), t.compact_of.end());
    const std::vector<unsigned long long> mask(t.lc_block_mask.begin(), t.lc_block_mask.end());
    c.K = t.K; c.Kc = t.Kc; c.P = t.P; c.method = method;
    c.T = t.T; c.tile_i = c.tile_j = 0;
    c.x = mem.put(t.x, stream); c.inv_x = mem.put(t.inv_x, stream);
    c.first_of = mem.put(first16, stream); c.compact_of = mem.put(comp16, stream);
    c.lut = mem.put(t.lut, stream); c.n_lut = static_cast<int>(t.lut.size() / 2);
    c.lc_block_mask = mem.put(mask, stream);
    // wide layout (33-64 pillars): the whole ladder in one launch when its LDS image fits, else one launch per tile pair
    c.wide_nch = cls.wide_nch;
    if (wide) {
        c.wide_ent = mem.put(t.wide_ent, stream); c.wide_store_map = mem.put(t.wide_store_map, stream);
        c.wide_pos = mem.put(t.wide_pos, stream); c.wide_order = mem.put(t.wide_order, stream);
        if (t.has_hess) c.wide_knot_chunks = mem.put(t.wide_knot_chunks, stream);
    }
    // the fast kernels store the [P][P] matrices as 16-byte pairs of the flat array: P must be even
    // LINEAR_FWD_RATES is linear in the knot DFs, not in their logs: only the general kernel carries the extra
    // Hessian term (kernels_general.hip, `Lookup`)
    c.packed_ok = cls.packed_ok;
    c.odd_last = t.odd_last;
    c.Pc = t.Pc; c.pc_pad = t.pc_pad; c.Ec = t.Ec; c.Eu = t.Eu; c.epg = t.epg; c.cpg = t.cpg; c.hub = t.hub ? 1 : 0;
    c.Kcore = t.Kcore; c.n_mini = t.n_mini; c.fringe_start = t.fringe_start; c.n_fringe = t.n_fringe; c.fringe_own = t.fringe_own ? 1 : 0;
    if (t.packed_ok) {
        c.knot_class = mem.put(t.knot_class, stream); c.pillar_to_core = mem.put(t.pillar_to_core, stream);
        c.out_map = mem.put(t.out_map, stream); c.store_map = mem.put(t.store_map, stream);
        c.ent_pq = mem.put(t.ent_pq, stream);
        c.core_pos = mem.put(t.core_pos, stream); c.lcc_pos = mem.put(t.lcc_pos, stream);
    }
    mem.note(hipStreamSynchronize(stream));       // (also on errors: the copies read this function's vectors)
}
}

struct adr_curve {
    adr_ctx* ctx = nullptr;
    adr::CurveDev dev{};
    R::CurveClass cls{};                 // what the launch plan reads (route.hpp)
    adr::DeviceOwner mem;
};

// Rate-independent description of one knot grid: its bootstrap scan and the table layout of the base curve.
struct adr_curve_plan {
    adr_ctx* ctx = nullptr;
    int interp = 0;
    bool has_hess = false;
    adr::CurveTables base;               // host tables of the base curve (structure + base values)
    adr::CurveBuildPlanDev dev{};
    adr::CurveDev shared{};              // the structural device arrays every built curve points at
    R::CurveClass cls{};                 // ... and the class of every built curve
    adr::DeviceOwner mem;
};

// Curves built together on the device; `curves` are views into the set's slabs.
struct adr_curve_set {
    adr_ctx* ctx = nullptr;
    const adr_curve_plan* plan = nullptr;
    int n = 0;
    double *dfs = nullptr, *jac = nullptr, *hess = nullptr;   // dense [n][K], [n][K][P], [n][K][P][P]
    std::vector<adr_curve> curves;
    adr::DeviceOwner mem;
};

struct adr_trades {
    adr_ctx* ctx = nullptr;
    adr::TradesDev dev{};            // the batch: headers and cash flows, the identity list, the plain row table
    int64_t n_fix_flows = 0, n_flt_flows = 0;
    // What each trade set of the launch plan (route.hpp, Set) hands its kernel: set[s] for the row tables (S_ROWS ..
    // S_LAGGED_CHAINED) and the trade lists (S_GENERAL .. S_ALL), lite[s] for the lite tables (S_LITE, S_LITE_LAG).
    adr::TradesDev set[R::kSets] = {};
    adr::LiteRowsDev lite[2] = {};
    R::TradeCounts counts;           // what the launch plan needs to know about the batch
    int64_t first_ratio = -1;        // the first trade with a ratio node (route.hpp, flag_lagged), -1 for none
    // per-wave stash of the payment-lag variant (kernels.hpp, OutputsDev::lag_scratch), sized for a grid of counts.lag_blocks
    // blocks.  It belongs to the BATCH (not to the ctx): two batches priced on two streams never share it.
    double* lag_scratch = nullptr;
    adr::DeviceOwner mem;

    // Schedule groups (schedule_groups.hpp).  The upload finds the groups and keeps them on the host;
    // the device tables of the groups in use under `mode` are (re)built by apply_schedule_groups - at upload and when
    // adr_trades_set_schedule_groups / _segment change a knob.  adr_price_dev only reads them.
    struct Grouping {
        adr::ScheduleGroups found;           // every group of at least two trades
        std::vector<int32_t> rows_order;     // the trades of the plain row table, in table order
        adr::CsrDev csr{};                   // the caller's arrays on the device (the ungrouped table is gathered from them)
        int mode = ADR_SCHEDULE_GROUPS_AUTO;
        int segment = 0;                     // records per wave of the store pass, 0: kScheduleSegment
        int blocks = 0;                      // 0: one wave per segment, else the size of a persistent grid
        bool active = false;
        int64_t used_groups = 0, used_trades = 0;
        adr::CombineDev combine{};
        adr::TradesDev basis{}, ungrouped{}; // row tables: two pseudo-trades per group / the plain rows outside the groups
        // An empty array is a real buffer here (the batch's own are null): when no group in use has a fixed leg, or none a
        // float leg, the basis batch has flow arrays of no elements, and its row builder and the fast kernel are handed
        // those pointers whatever the counts; that neither ever forms a read from a null one has not been shown.
        adr::DeviceOwner mem{true};
        // Releases the device tables: no grouped route.  Returns the error the owner held.
        hipError_t reset() {
            active = false;
            used_groups = used_trades = 0;
            combine = adr::CombineDev{};
            return mem.release();
        }
    } grouping;

    // The plan of the last (curve class, request) this batch was priced with: built on first use, replayed afterwards.  A
    // caller gets a reference-counted immutable plan, taken under the lock: a concurrent call with another request replaces
    // the cached pointer, never the plan the caller is walking.
    struct PlanKey { R::CurveClass cls; int req[4]; };
    mutable std::mutex plan_mutex;
    mutable PlanKey plan_key{};
    mutable std::shared_ptr<const R::Plan> plan;
    std::shared_ptr<const R::Plan> plan_for(const R::CurveClass& cls, bool want_delta, bool want_gamma, bool per_trade, bool has_agg,
                                            int n_cu) const {
        PlanKey key{};
        key.cls = cls;
        key.req[0] = want_delta; key.req[1] = want_gamma; key.req[2] = per_trade; key.req[3] = has_agg;
        std::lock_guard<std::mutex> lock(plan_mutex);
        if (!plan || std::memcmp(&key, &plan_key, sizeof key) != 0) {
            plan = std::make_shared<const R::Plan>(R::make_plan(cls, counts, want_delta, want_gamma, per_trade, has_agg, n_cu));
            plan_key = key;
        }
        return plan;
    }
};

// the host-only translation units (book_host.cpp) report errors through the same per-thread message
int adr_set_error(int status, const std::string& msg) { return fail(status, msg); }

// the GPU and stream of a ctx, for the launch code of other translation units (bond_measures.hip, frn_measures.hip)
int adr_ctx_target(const adr_ctx* ctx, int* device, hipStream_t* stream) {
    if (!ctx) return fail(ADR_ERR_INVALID, "null ctx");
    *device = ctx->device;
    *stream = ctx->stream;
    return ADR_OK;
}

// what scenario_pv.hip needs of the opaque handles: the ctx's compute units, a batch's device arrays and a curve set's
// dense arrays (knot times [K], discount factors [S][K])
int adr_ctx_compute_units(const adr_ctx* ctx) { return ctx ? ctx->n_cu : 0; }

const adr::TradesDev* adr_trades_device_view(const adr_trades* trades, const adr_ctx** owner) {
    if (!trades) return nullptr;
    *owner = trades->ctx;
    return &trades->dev;
}

// what subbook_ladder.hip needs: a curve's tables and the first trade of a batch that has a ratio node (-1: none)
const adr::CurveDev* adr_curve_device_view(const adr_curve* curve, const adr_ctx** owner) {
    if (!curve) return nullptr;
    *owner = curve->ctx;
    return &curve->dev;
}

int64_t adr_trades_first_ratio(const adr_trades* trades) { return trades ? trades->first_ratio : -1; }

int adr_curve_set_device_view(const adr_curve_set* set, const adr_ctx** owner, int* method, int* K, int* S,
                              const double** times_dev, const double** dfs_dev) {
    if (!set || !set->plan) return fail(ADR_ERR_INVALID, "null curve set");
    *owner = set->ctx;
    *method = set->plan->interp;
    *K = set->plan->base.K;
    *S = set->n;
    *times_dev = set->plan->shared.x;
    *dfs_dev = set->dfs;
    return ADR_OK;
}

// what curve_dfs.hip needs of a curve plan: its owner and the scan arrays on the device
int adr_curve_plan_scan_view(const adr_curve_plan* plan, const adr_ctx** owner, int* K, int* P, const double** acc_dev,
                             const int32_t** pillar_dev, const int32_t** prev_idx_dev) {
    if (!plan) return fail(ADR_ERR_INVALID, "null curve plan");
    *owner = plan->ctx;
    *K = plan->dev.K;
    *P = plan->dev.P;
    *acc_dev = plan->dev.acc;
    *pillar_dev = plan->dev.pillar;
    *prev_idx_dev = plan->dev.prev_idx;
    return ADR_OK;
}

extern "C" {

int adr_version(void) { return 100; }

const char* adr_last_error(void) { return g_last_error.c_str(); }

int adr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int adr_init(int device_ordinal, adr_ctx** out) {
    if (!out) return fail(ADR_ERR_INVALID, "adr_init: out is null");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(ADR_ERR_HIP, "adr_init: no HIP device available (this library has no CPU fallback)");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(ADR_ERR_INVALID, "adr_init: bad device ordinal");
    ADR_HIP(hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    ADR_HIP(hipGetDeviceProperties(&prop, device_ordinal));
    adr_ctx* ctx = new (std::nothrow) adr_ctx();
    if (!ctx) return fail(ADR_ERR_NOMEM, "adr_init: out of memory");
    ctx->device = device_ordinal;
    ctx->n_cu = prop.multiProcessorCount;
    ctx->lds_limit = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor
                                                           : prop.sharedMemPerBlock;
    // (every failure from here on releases what the ctx holds so far through adr_free_ctx, which tests each member)
    e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { adr_free_ctx(ctx); return fail_hip(e, "hipStreamCreate"); }
    const R::Grid grid = R::grid_for(ctx->n_cu);
    ctx->max_blocks = grid.max_blocks;
    e = hipMalloc(reinterpret_cast<void**>(&ctx->partials),
                  sizeof(double) * static_cast<size_t>(ctx->max_blocks) * adr::kAggStride);
    if (e != hipSuccess) { adr_free_ctx(ctx); return fail_hip(e, "hipMalloc(partials)"); }
    e = hipMalloc(reinterpret_cast<void**>(&ctx->dump), sizeof(double) * adr::kPillarPad * adr::kPillarPad);
    if (e != hipSuccess) { adr_free_ctx(ctx); return fail_hip(e, "hipMalloc(dump)"); }
    ctx->knot_blocks = grid.knot_blocks;
    e = hipMalloc(reinterpret_cast<void**>(&ctx->knot_partials),
                  sizeof(double) * (static_cast<size_t>(ctx->knot_blocks + 1) * kKnotStrideMax + static_cast<size_t>(R::kKnotLagMaxKc) * R::kKnotLagMaxKc + 1));
    if (e != hipSuccess) { adr_free_ctx(ctx); return fail_hip(e, "hipMalloc(knot partials)"); }
    ctx->knot_reduced = ctx->knot_partials + static_cast<size_t>(ctx->knot_blocks) * kKnotStrideMax;
    ctx->knot_overflow = ctx->knot_reduced + kKnotStrideMax;
    // Dynamic-LDS ceiling of every kernel instantiation, once per device: the whole 160 KiB of a CU.  (Setting it per
    // uploaded curve to that curve's need would LOWER it below what an earlier, larger curve's launches request.)
    e = adr::set_kernel_lds_limits(kLdsBudget, kLdsBudget);
    if (e != hipSuccess) { adr_free_ctx(ctx); return fail_hip(e, "hipFuncSetAttribute(MaxDynamicSharedMemorySize)"); }
#ifdef ADR_STAMPS
    hipMalloc(reinterpret_cast<void**>(&ctx->stamps), sizeof(unsigned long long) * ctx->max_blocks * 16 * 8);
    hipMemset(ctx->stamps, 0, sizeof(unsigned long long) * ctx->max_blocks * 16 * 8);
#endif
    *out = ctx;
    return ADR_OK;
}

#ifdef ADR_STAMPS
extern "C" int adr_debug_stamps(adr_ctx* ctx, unsigned long long* host, int n_waves) {
    hipDeviceSynchronize();
    return hipMemcpy(host, ctx->stamps, sizeof(unsigned long long) * n_waves * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -3;
}
#endif

void adr_free_ctx(adr_ctx* ctx) {
    if (!ctx) return;
    hipSetDevice(ctx->device);
    if (ctx->partials) hipFree(ctx->partials);
    if (ctx->dump) hipFree(ctx->dump);
    if (ctx->knot_partials) hipFree(ctx->knot_partials);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
}

int adr_sync(adr_ctx* ctx) {
    if (!ctx) return fail(ADR_ERR_INVALID, "adr_sync: ctx is null");
    ADR_HIP(hipStreamSynchronize(ctx->stream));
    return ADR_OK;
}

// ------------------------------------------------------------------------------------------- curve
int adr_curve_tables_host(int K, int P, const double* times, const double* dfs, const double* jac,
                          const double* hess, int32_t* knot_index, double* log_df, double* lj, double* lc) {
    adr::CurveTables t;
    const std::string err = adr::build_curve_tables(K, P, times, dfs, jac, hess, t);
    if (!err.empty()) return fail(ADR_ERR_INVALID, "adr_curve_tables_host: " + err);
    if (knot_index) std::copy(t.knot_index.begin(), t.knot_index.end(), knot_index);
    if (log_df) std::copy(t.log_df.begin(), t.log_df.end(), log_df);
    if (lj)
        for (int c = 0; c < t.Kc; ++c)
            for (int p = 0; p < P; ++p)
                lj[static_cast<size_t>(c) * P + p] =
                    t.lj[(static_cast<size_t>(p / adr::kPillarPad) * t.Kc + c) * adr::kPillarPad + p % adr::kPillarPad];
    if (lc && t.has_hess) std::copy(t.lc.begin(), t.lc.end(), lc);
    return t.Kc;
}

int adr_curve_layout_host(int K, int P, const double* times, const double* dfs, const double* jac,
                          const double* hess, int64_t* info) {
    if (!info) return fail(ADR_ERR_INVALID, "adr_curve_layout_host: info is null");
    adr::CurveTables t;
    const std::string err = adr::build_curve_tables(K, P, times, dfs, jac, hess, t);
    if (!err.empty()) return fail(ADR_ERR_INVALID, "adr_curve_layout_host: " + err);
    const R::CurveClass cls = R::curve_class(t, 0, false);
    info[0] = t.packed_ok ? 1 : 0; info[1] = t.Pc; info[2] = t.Ec; info[3] = t.Eu; info[4] = t.epg;
    info[5] = t.Kcore; info[6] = t.n_mini;
    info[7] = t.packed_ok ? static_cast<int64_t>(adr::fast_kernel_lds_bytes(cls.sizes(), t.has_hess)) : 0;
    // the general kernel's variant with LDS-resident convexity rows (it serves what the fast kernels do not take)
    info[8] = (t.packed_ok && t.has_hess && t.T == 1)
        ? static_cast<int64_t>(adr::general_lds_kernel_lds_bytes_for(t.K, t.Kc, t.Kcore, t.Ec, t.n_mini, cls.n_lut, true)) : 0;
    info[9] = cls.lds_rows;
    info[10] = t.cpg;
    info[11] = t.hub ? 1 : 0;
    info[12] = t.wide_nch;
    info[13] = t.wide_nch > 0 ? static_cast<int64_t>(adr::wide_kernel_lds_bytes(t.K, t.Kc, t.wide_nch, t.has_hess)) : 0;
    info[14] = 0;
    for (uint32_t m : t.wide_knot_chunks) info[14] = std::max<int64_t>(info[14], __builtin_popcount(m));
    info[15] = static_cast<int64_t>(adr::general_kernel_lds_bytes(t.K, t.Kc, t.T > 1));   // what adr_curve_upload checks
    return ADR_OK;
}

void adr_free_curve(adr_curve* curve) {
    if (!curve) return;
    if (curve->ctx) hipSetDevice(curve->ctx->device);
    curve->mem.release();
    delete curve;
}

int adr_curve_pillars(const adr_curve* curve) { return curve ? curve->dev.P : 0; }

int adr_curve_upload(adr_ctx* ctx, int interp_method, int K, int P, const double* times, const double* dfs,
                     const double* jac, const double* hess, adr_curve** out) {
    return adr_curve_upload_ex(ctx, interp_method, K, P, times, dfs, jac, hess, 0u, out);
}

int adr_curve_upload_ex(adr_ctx* ctx, int interp_method, int K, int P, const double* times, const double* dfs,
                        const double* jac, const double* hess, uint32_t flags, adr_curve** out) {
    if (!ctx || !out) return fail(ADR_ERR_INVALID, "adr_curve_upload: null ctx/out");
    *out = nullptr;
    if (flags & ~static_cast<uint32_t>(ADR_CURVE_PILLAR_TILES))
        return fail(ADR_ERR_INVALID, "adr_curve_upload_ex: unknown flag bits");
    if (const int rc = check_interp(interp_method, "adr_curve_upload")) return rc;
    if (P > ADR_MAX_PILLARS)
        return fail(ADR_ERR_UNSUPPORTED, "adr_curve_upload: more than ADR_MAX_PILLARS (256) pillars");
    adr::CurveTables t;
    const std::string err = adr::build_curve_tables(K, P, times, dfs, jac, hess, t);
    if (!err.empty()) return fail(ADR_ERR_INVALID, "adr_curve_upload: " + err);

    const size_t lds = adr::general_kernel_lds_bytes(t.K, t.Kc, t.T > 1);
    if (lds > kLdsBudget)
        return fail(ADR_ERR_UNSUPPORTED, "adr_curve_upload: curve tables exceed the 160 KiB LDS of a CU");

    ADR_HIP(hipSetDevice(ctx->device));
    adr_curve* c = new (std::nothrow) adr_curve();
    if (!c) return fail(ADR_ERR_NOMEM, "adr_curve_upload: out of memory");
    c->ctx = ctx;
    c->cls = R::curve_class(t, interp_method, (flags & ADR_CURVE_PILLAR_TILES) != 0);
    adr::DeviceOwner& mem = c->mem;
    adr::CurveDev& d = c->dev;
    hipStream_t stream = ctx->stream;
    // The value arrays; the structural half last, because it waits for the stream: `t` outlives every copy, and the curve
    // is returned only with its tables on the device.
    d.log_df = mem.put(t.log_df, stream); d.lj = mem.put(t.lj, stream); d.lc_lanes = mem.put(t.lc_lanes, stream);
    const bool wide = c->cls.wide_nch > 0;
    if (wide) {
        d.lj64 = mem.put(t.lj64, stream);
        if (t.has_hess) d.lcflat = mem.put(t.lcflat, stream);
    }
    if (t.packed_ok) { d.ljc = mem.put(t.ljc, stream); d.lcc = mem.put(t.lcc, stream); d.mini = mem.put(t.mini, stream); }
    fill_curve_structure(t, interp_method, c->cls, wide, mem, stream, d);
    if (!mem.ok()) {
        const hipError_t e = mem.error;
        adr_free_curve(c);
        return fail_hip(e, "adr_curve_upload: copying tables");
    }
    *out = c;
    return ADR_OK;
}

// ------------------------------------------------------------------------------ batched curve lookups
int adr_curve_df_dev(adr_ctx* ctx, const adr_curve* curve, int64_t n, const double* t_dev, double* df_dev, void* stream_v) {
    if (!ctx || !curve) return fail(ADR_ERR_INVALID, "adr_curve_df: null ctx/curve");
    if (curve->ctx != ctx) return fail(ADR_ERR_INVALID, "adr_curve_df: the curve was uploaded through another ctx");
    if (n < 0 || (n > 0 && (!t_dev || !df_dev))) return fail(ADR_ERR_INVALID, "adr_curve_df: bad count / null array");
    ADR_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = stream_v ? static_cast<hipStream_t>(stream_v) : ctx->stream;
    ADR_HIP(adr::launch_curve_df(curve->dev, n, t_dev, df_dev, ctx->n_cu, stream));
    return ADR_OK;
}

int adr_curve_df(adr_ctx* ctx, const adr_curve* curve, int64_t n, const double* t, double* df) {
    if (!ctx || !curve) return fail(ADR_ERR_INVALID, "adr_curve_df: null ctx/curve");
    if (n < 0 || (n > 0 && (!t || !df))) return fail(ADR_ERR_INVALID, "adr_curve_df: bad count / null array");
    if (n == 0) return ADR_OK;
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(t[i])) return fail(ADR_ERR_INVALID, "adr_curve_df: times must be finite");
    ADR_HIP(hipSetDevice(ctx->device));
    adr::DeviceOwner tmp;                     // the call's two device arrays
    double* d_t = tmp.put_n(t, static_cast<size_t>(n), ctx->stream);
    double* d_df = tmp.array<double>(static_cast<size_t>(n));
    int rc = ADR_OK;
    if (tmp.ok()) rc = adr_curve_df_dev(ctx, curve, n, d_t, d_df, nullptr);
    if (tmp.ok() && rc == ADR_OK)
        tmp.note(hipMemcpyAsync(df, d_df, sizeof(double) * static_cast<size_t>(n), hipMemcpyDeviceToHost, ctx->stream));
    if (tmp.ok() && rc == ADR_OK) tmp.note(hipStreamSynchronize(ctx->stream));
    const hipError_t e = tmp.release();
    if (rc != ADR_OK) return rc;
    if (e != hipSuccess) return fail_hip(e, "adr_curve_df");
    return ADR_OK;
}

// ------------------------------------------------------------------------------ device curve builder
void adr_free_curve_plan(adr_curve_plan* plan) {
    if (!plan) return;
    if (plan->ctx) hipSetDevice(plan->ctx->device);
    plan->mem.release();
    delete plan;
}

int adr_curve_plan_create(adr_ctx* ctx, int interp_method, int K, int P, const double* times, const double* acc,
                          const int32_t* pillar, const int32_t* prev_idx, const double* base_dfs,
                          const double* base_jac, const double* base_hess, adr_curve_plan** out) {
    if (!ctx || !out) return fail(ADR_ERR_INVALID, "adr_curve_plan_create: null ctx/out");
    *out = nullptr;
    if (const int rc = check_interp(interp_method, "adr_curve_plan_create")) return rc;
    if (P > ADR_MAX_PLAN_PILLARS)
        return fail(ADR_ERR_UNSUPPORTED, "adr_curve_plan_create: more than ADR_MAX_PLAN_PILLARS (64) pillars");
    if (!acc || !pillar || !prev_idx) return fail(ADR_ERR_INVALID, "adr_curve_plan_create: null scan arrays");
    for (int k = 0; k < K; ++k) {
        if (pillar[k] < 0 || pillar[k] >= P) return fail(ADR_ERR_INVALID, "adr_curve_plan_create: pillar index out of range");
        if (prev_idx[k] < -1 || prev_idx[k] >= K) return fail(ADR_ERR_INVALID, "adr_curve_plan_create: prev_idx out of range");
    }
    adr_curve_plan* plan = new (std::nothrow) adr_curve_plan();
    if (!plan) return fail(ADR_ERR_NOMEM, "adr_curve_plan_create: out of memory");
    plan->ctx = ctx;
    plan->interp = interp_method;
    plan->has_hess = base_hess != nullptr;
    adr::CurveTables& t = plan->base;
    const std::string err = adr::build_curve_tables(K, P, times, base_dfs, base_jac, base_hess, t);
    if (!err.empty()) { delete plan; return fail(ADR_ERR_INVALID, "adr_curve_plan_create: " + err); }
    // more than 32 pillars: the built curves carry the wide layout's tables only (no tiled route for them).  (Every curve this
    // accepts - at most 64 pillars, wide tables that fit the LDS - is one curve_class puts on the wide route.)
    const bool wide = t.T > 1;
    const size_t lds = wide ? adr::wide_kernel_lds_bytes(t.K, t.Kc, t.wide_nch, plan->has_hess) : adr::general_kernel_lds_bytes(t.K, t.Kc);
    // the PV01 gradients of the scan ([K][P] doubles) stay in LDS when they fit, else they go through a scratch buffer
    const bool dpv_global = adr::bootstrap_kernel_lds_bytes(K, P, false) > kLdsBudget;
    if (lds > kLdsBudget || adr::bootstrap_kernel_lds_bytes(K, P, dpv_global) > kLdsBudget) {
        delete plan;
        return fail(ADR_ERR_UNSUPPORTED, "adr_curve_plan_create: curve tables exceed the 160 KiB LDS of a CU");
    }
    hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) { delete plan; return fail_hip(e, "hipSetDevice"); }

    std::vector<int32_t> core_pillars;
    for (int p = 0; p < P; ++p)
        if (t.packed_ok && t.pillar_to_core[p] < t.Pc) core_pillars.push_back(p);
    adr::DeviceOwner& mem = plan->mem;
    hipStream_t stream = ctx->stream;
    R::CurveClass& cls = plan->cls;
    cls = R::curve_class(t, interp_method, false);
    if (!cls.packed_ok) cls.lds_rows = 0;   // (the built curves carry the convexity rows only with the packed layout)
    // The scan arrays, read from the caller's; the structural half last, because it waits for the stream: the caller's
    // arrays, `core_pillars` and the plan's tables outlive every copy.
    adr::CurveBuildPlanDev& d = plan->dev;
    d.K = K; d.P = P; d.Kc = t.Kc;
    d.acc = mem.put_n(acc, static_cast<size_t>(K), stream); d.pillar = mem.put_n(pillar, static_cast<size_t>(K), stream);
    d.prev_idx = mem.put_n(prev_idx, static_cast<size_t>(K), stream); d.knot_index = mem.put(t.knot_index, stream);
    d.packed_ok = cls.packed_ok;
    d.Pc = t.Pc; d.pc_pad = t.pc_pad; d.Ec = t.Ec; d.Kcore = t.Kcore; d.n_mini = t.n_mini;
    d.wide_nch = cls.wide_nch; d.dpv_global = dpv_global ? 1 : 0;
    if (wide) d.wide_pq = mem.put(t.wide_pq, stream);
    if (t.packed_ok) { d.core_pillars = mem.put(core_pillars, stream); d.lcc_pq = mem.put(t.lcc_pq, stream); }
    fill_curve_structure(t, interp_method, cls, wide, mem, stream, plan->shared);
    d.knot_class = plan->shared.knot_class;
    if (!mem.ok()) {
        e = mem.error;
        adr_free_curve_plan(plan);
        return fail_hip(e, "adr_curve_plan_create: copying tables");
    }
    *out = plan;
    return ADR_OK;
}

void adr_free_curve_set(adr_curve_set* set) {
    if (!set) return;
    if (set->ctx) hipSetDevice(set->ctx->device);
    set->mem.release();
    delete set;
}

int adr_curve_set_size(const adr_curve_set* set) { return set ? set->n : 0; }

const adr_curve* adr_curve_set_get(const adr_curve_set* set, int i) {
    if (!set || i < 0 || i >= set->n) { fail(ADR_ERR_INVALID, "adr_curve_set_get: index out of range"); return nullptr; }
    return &set->curves[static_cast<size_t>(i)];
}

int adr_curve_set_build(adr_ctx* ctx, const adr_curve_plan* plan, int n_scen, const double* rates,
                        adr_curve_set** out) {
    if (!ctx || !plan || !out) return fail(ADR_ERR_INVALID, "adr_curve_set_build: null ctx/plan/out");
    *out = nullptr;
    if (n_scen < 0 || (n_scen > 0 && !rates)) return fail(ADR_ERR_INVALID, "adr_curve_set_build: bad scenario count / null rates");
    const adr::CurveTables& t = plan->base;
    const size_t S = static_cast<size_t>(n_scen), K = t.K, P = t.P, Kc = t.Kc;
    for (size_t i = 0; i < S * P; ++i)
        if (!std::isfinite(rates[i])) return fail(ADR_ERR_INVALID, "adr_curve_set_build: par rates must be finite");
    ADR_HIP(hipSetDevice(ctx->device));
    adr_curve_set* set = new (std::nothrow) adr_curve_set();
    if (!set) return fail(ADR_ERR_NOMEM, "adr_curve_set_build: out of memory");
    set->ctx = ctx; set->plan = plan; set->n = n_scen;
    if (n_scen == 0) { *out = set; return ADR_OK; }

    // The set's slabs, one per table with a leading scenario axis (null for an absent table); those the build adds into
    // or leaves partly unwritten are zeroed.
    adr::DeviceOwner& mem = set->mem;
    hipStream_t stream = ctx->stream;
    const bool hs = plan->has_hess, packed = plan->dev.packed_ok != 0;
    double* d_rates = mem.put_n(rates, S * P, stream);
    set->dfs = mem.array<double>(S * K);
    set->jac = mem.array<double>(S * K * P);
    set->hess = hs ? mem.array<double>(S * K * P * P) : nullptr;
    adr::CurvePackOut po{};
    po.log_df = mem.array<double>(S * Kc);
    const bool wide = plan->dev.wide_nch > 0;
    const size_t wrow = static_cast<size_t>(plan->dev.wide_nch) * adr::kWideChunk;
    if (wide) {
        po.lj64 = mem.array<double>(S * Kc * adr::kWidePad);
        po.lcflat = hs ? static_cast<double*>(mem.alloc_zeroed(sizeof(double) * S * Kc * wrow, stream)) : nullptr;
    } else {
        po.lj = mem.array<double>(S * Kc * adr::kPillarPad);
        po.lc_lanes = hs ? mem.array<double>(S * Kc * 64 * adr::kGammaPerLane) : nullptr;
    }
    const size_t ljc_n = static_cast<size_t>(t.Kcore + 1) * t.pc_pad, lcc_n = static_cast<size_t>(t.Kcore + 1) * (t.Ec + 1);
    if (packed) {
        po.ljc = static_cast<double*>(mem.alloc_zeroed(sizeof(double) * S * ljc_n, stream));
        po.lcc = hs ? static_cast<double*>(mem.alloc_zeroed(sizeof(double) * S * lcc_n, stream)) : nullptr;
        po.mini = mem.array<adr::MiniKnot>(S * std::max(1, t.n_mini));
    }
    // scratch of the scan's second-derivative state; released once the build has run
    adr::DeviceOwner tmp;
    double* d_scratch = hs && mem.ok() ? tmp.array<double>(S * K * P * P) : nullptr;
    double* d_dpv = plan->dev.dpv_global && mem.ok() ? tmp.array<double>(S * K * P) : nullptr;
    mem.note(tmp.error);
    if (packed && t.n_mini > 0)
        for (size_t s = 0; s < S && mem.ok(); ++s)   // pillar / entry fields of the short-end records
            mem.note(hipMemcpyAsync(po.mini + s * t.n_mini, t.mini.data(), sizeof(adr::MiniKnot) * t.n_mini,
                                    hipMemcpyHostToDevice, stream));
    if (mem.ok())
        mem.note(adr::launch_curve_build(plan->dev, n_scen, d_rates, set->dfs, set->jac, set->hess, d_scratch, d_dpv, po, stream));
    mem.note(hipStreamSynchronize(stream));      // (also on errors: the copies read the caller's rates)
    tmp.release();
    if (!mem.ok()) {
        const hipError_t e = mem.error;
        adr_free_curve_set(set);
        return fail_hip(e, "adr_curve_set_build");
    }

    set->curves.resize(S);
    for (size_t s = 0; s < S; ++s) {
        adr_curve& c = set->curves[s];
        c.ctx = ctx;
        c.dev = plan->shared;
        c.cls = plan->cls;
        c.dev.log_df = po.log_df + s * Kc;
        if (wide) {
            c.dev.lj64 = po.lj64 + s * Kc * adr::kWidePad;
            c.dev.lcflat = hs ? po.lcflat + s * Kc * wrow : nullptr;
        } else {
            c.dev.lj = po.lj + s * Kc * adr::kPillarPad;
            c.dev.lc_lanes = hs ? po.lc_lanes + s * Kc * 64 * adr::kGammaPerLane : nullptr;
        }
        if (packed) {
            c.dev.ljc = po.ljc + s * ljc_n;
            c.dev.lcc = hs ? po.lcc + s * lcc_n : nullptr;
            c.dev.mini = po.mini + s * t.n_mini;
        }
    }
    *out = set;
    return ADR_OK;
}

int adr_curve_set_download(const adr_curve_set* set, int i, double* dfs, double* jac, double* hess) {
    if (!set || i < 0 || i >= set->n) return fail(ADR_ERR_INVALID, "adr_curve_set_download: index out of range");
    const size_t K = set->plan->base.K, P = set->plan->base.P, s = static_cast<size_t>(i);
    ADR_HIP(hipSetDevice(set->ctx->device));
    if (dfs) ADR_HIP(hipMemcpy(dfs, set->dfs + s * K, sizeof(double) * K, hipMemcpyDeviceToHost));
    if (jac) ADR_HIP(hipMemcpy(jac, set->jac + s * K * P, sizeof(double) * K * P, hipMemcpyDeviceToHost));
    if (hess) {
        if (!set->hess) return fail(ADR_ERR_INVALID, "adr_curve_set_download: the plan was created without hess");
        ADR_HIP(hipMemcpy(hess, set->hess + s * K * P * P, sizeof(double) * K * P * P, hipMemcpyDeviceToHost));
    }
    return ADR_OK;
}

// ------------------------------------------------------------------------------------------ trades
void adr_free_trades(adr_trades* t) {
    if (!t) return;
    if (t->ctx) hipSetDevice(t->ctx->device);
    t->grouping.mem.release();
    t->mem.release();
    delete t;
}

}  // extern "C"

namespace {

// Policy of the grouped route under ADR_SCHEDULE_GROUPS_AUTO, both measured ("policy"): a group is
// used from kScheduleMinGroup trades on (its two basis walks and their 16 KB of ladders against the walks its members no
// longer make: on 262 144 trades in equal groups the route is 1 % slower than the direct one at 32 per group and 7 % faster
// at 64), a batch takes the route from kScheduleMinGrouped such trades on (three more launches: slower at 16 384, faster at
// 32 768).  FORCE: every group of two or more, whatever the batch size.
constexpr int kScheduleMinGroup = 64;
constexpr int64_t kScheduleMinGrouped = 32768;
constexpr int kScheduleSegment = 16;         // records per wave of the store pass (kernels_combine.hip)

// One row table of the fast kernel (kernels.hpp): 32 zero-padded slots per row and array, gathered on the device
// (trades_build.hip) from the work list - `piece_trade`: the row's trade, or -1 for an empty row; a chained table also has
// `piece_first` (first coupon of the piece) and `piece_more` ("the trade continues"), any other passes null for both.  Fills
// the row fields of `dst` and nothing else of it; an empty list is a table of no rows and launches nothing.  The lists must
// outlive the copies (DeviceOwner::put).
void build_row_table(const adr::CsrDev& csr, const std::vector<int32_t>& piece_trade, const std::vector<int32_t>* piece_first,
                     const std::vector<uint8_t>* piece_more, bool lagged, bool weighted, adr::DeviceOwner& mem, hipStream_t stream,
                     adr::TradesDev& dst) {
    dst.n_rows = 0;
    if (piece_trade.empty()) return;
    const size_t rows = piece_trade.size(), S = adr::kRowSlots;
    adr::RowBuildDev rb{};
    rb.rows = static_cast<int64_t>(rows);
    rb.piece_trade = mem.put(piece_trade, stream, kBatchPad);
    rb.piece_first = piece_first ? mem.put(*piece_first, stream, kBatchPad) : nullptr;
    rb.piece_more = piece_more ? mem.put(*piece_more, stream, kBatchPad) : nullptr;
    rb.row_tp = mem.array<double>(rows * S, kBatchPad);
    rb.row_ts = mem.array<double>(rows * S, kBatchPad);
    rb.row_alpha = mem.array<double>(rows * S, kBatchPad);
    rb.row_xtp = mem.array<double>(rows * S, kBatchPad);
    rb.row_xpay = mem.array<double>(rows * S, kBatchPad);
    rb.row_te = lagged ? mem.array<double>(rows * S, kBatchPad) : nullptr;
    rb.row_w = (lagged && weighted) ? mem.array<double>(rows * S, kBatchPad) : nullptr;
    rb.row_notional = mem.array<double>(rows, kBatchPad);
    rb.row_spread = mem.array<double>(rows, kBatchPad);
    rb.row_meta = mem.array<int32_t>(rows, kBatchPad);
    rb.row_trade = mem.array<int32_t>(rows, kBatchPad);
    if (mem.ok()) mem.note(adr::launch_build_rows(csr, rb, stream));
    dst.n_rows = static_cast<int64_t>(rows);
    dst.row_tp = rb.row_tp; dst.row_ts = rb.row_ts; dst.row_alpha = rb.row_alpha; dst.row_xtp = rb.row_xtp; dst.row_xpay = rb.row_xpay;
    dst.row_notional = rb.row_notional; dst.row_spread = rb.row_spread; dst.row_meta = rb.row_meta; dst.row_trade = rb.row_trade;
    dst.rows_chained = piece_first ? 1 : 0;
    dst.rows_lagged = lagged ? 1 : 0;
    dst.row_te = rb.row_te; dst.row_w = rb.row_w;
}

// (Re)builds the device tables of the batch's schedule groups for its current knobs: the host image of the groups in use
// (schedule_groups.hpp, build_group_tables), uploaded.  Allocates and synchronises: never called from adr_price_dev, and not
// while a pricing call on the batch is in flight.
hipError_t apply_schedule_groups(adr_trades* tr) {
    adr_trades::Grouping& G = tr->grouping;
    adr::DeviceOwner& mem = G.mem;
    hipStream_t stream = tr->ctx->stream;
    const hipError_t e0 = hipStreamSynchronize(stream);       // first: nothing on the stream reads the tables released next
    G.reset();
    if (e0 != hipSuccess) return e0;
    if (G.mode == ADR_SCHEDULE_GROUPS_OFF || G.found.n_groups == 0) return hipSuccess;
    const bool force = G.mode == ADR_SCHEDULE_GROUPS_FORCE;
    const adr::GroupTables T = adr::build_group_tables(G.found, G.rows_order.data(), static_cast<int64_t>(G.rows_order.size()),
                                                       force ? 2 : kScheduleMinGroup, force ? 0 : kScheduleMinGrouped,
                                                       G.segment > 0 ? G.segment : kScheduleSegment);
    if (T.used_groups == 0) return hipSuccess;             // route not taken
    const size_t ng = static_cast<size_t>(T.used_groups);

    G.ungrouped = tr->dev;
    build_row_table(G.csr, T.rest, nullptr, nullptr, false, false, mem, stream, G.ungrouped);
    adr::CsrDev bc{};
    bc.n = static_cast<int64_t>(2 * ng);
    bc.fix_off = mem.put(T.fix_off, stream, kBatchPad); bc.flt_off = mem.put(T.flt_off, stream, kBatchPad);
    bc.fix_tp = mem.put(T.fix_tp, stream, kBatchPad); bc.fix_pay = mem.put(T.fix_pay, stream, kBatchPad);
    bc.flt_tp = mem.put(T.flt_tp, stream, kBatchPad); bc.flt_ts = mem.put(T.flt_ts, stream, kBatchPad);
    bc.flt_te = mem.put(T.flt_te, stream, kBatchPad); bc.flt_alpha = mem.put(T.flt_alpha, stream, kBatchPad);
    bc.notional = mem.put(T.notional, stream, kBatchPad); bc.spread = mem.put(T.spread, stream, kBatchPad);
    bc.fix_sign = mem.put(T.sign, stream, kBatchPad); bc.flt_sign = mem.put(T.sign, stream, kBatchPad);
    G.basis = tr->dev;
    build_row_table(bc, T.rows, nullptr, nullptr, false, false, mem, stream, G.basis);
    G.basis.n = bc.n;

    adr::CombineDev& cd = G.combine;
    cd.rec = mem.put(T.rec, stream, kBatchPad);
    cd.seg = mem.put(T.seg, stream, kBatchPad);
    cd.n_seg = static_cast<int64_t>(T.seg.size());
    cd.max_blocks = G.blocks;
    cd.n_groups = T.used_groups;
    cd.sum_f = mem.put(T.sum_f, stream, kBatchPad); cd.sum_x = mem.put(T.sum_x, stream, kBatchPad);
    // the basis ladders of a pricing call, for any curve of up to 32 pillars
    constexpr size_t PM = adr::kPillarPad;
    cd.b_pv = mem.array<double>(2 * ng, kBatchPad);
    cd.b_delta = mem.array<double>(2 * ng * PM, kBatchPad);
    cd.b_gamma = mem.array<double>(2 * ng * PM * PM, kBatchPad);
    mem.note(hipStreamSynchronize(stream));                    // (also on errors: the copies read `T`)
    if (!mem.ok()) return G.reset();
    G.used_groups = T.used_groups;
    G.used_trades = T.used_trades;
    G.active = true;
    return hipSuccess;
}

// Which table or list every trade lands in, and the host side of those tables (route.cpp), with the one limit they have.
// `flagged`: the caller has filled lagged_of (the upload does, in its parallel validation pass); else the trades with
// payment lag or per-coupon notionals are flagged here (route.hpp, flag_lagged).  `who`: the entry point, for the message.
int layout_trades(const char* who, int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* flt_tp,
                  const double* flt_te, const double* flt_alpha, const double* flt_weight, int n_cu, bool flagged,
                  std::vector<uint8_t>& lagged_of, R::TradeLayout& L) {
    if (!flagged) {
        lagged_of.assign(static_cast<size_t>(n), 0);
        R::flag_lagged(0, n, flt_off, flt_tp, flt_te, flt_alpha, flt_weight, lagged_of.data());
    }
    L = R::trade_layout(n, fix_off, flt_off, lagged_of.data(), n_cu);
    if (L.too_many_rows)
        return fail(ADR_ERR_UNSUPPORTED, std::string(who) + ": more than 2^28 rows in the delta-only table; shard the portfolio");
    return ADR_OK;
}

}  // namespace

extern "C" {

int adr_trades_set_schedule_groups(adr_trades* trades, int mode) {
    if (!trades) return fail(ADR_ERR_INVALID, "adr_trades_set_schedule_groups: null batch");
    if (mode != ADR_SCHEDULE_GROUPS_AUTO && mode != ADR_SCHEDULE_GROUPS_OFF && mode != ADR_SCHEDULE_GROUPS_FORCE)
        return fail(ADR_ERR_INVALID, "adr_trades_set_schedule_groups: mode must be AUTO, OFF or FORCE");
    ADR_HIP(hipSetDevice(trades->ctx->device));
    trades->grouping.mode = mode;
    ADR_HIP(apply_schedule_groups(trades));
    return ADR_OK;
}

int adr_trades_set_schedule_segment(adr_trades* trades, int records, int blocks) {
    if (!trades || records < 0 || blocks < 0) return fail(ADR_ERR_INVALID, "adr_trades_set_schedule_segment: null batch / negative argument");
    ADR_HIP(hipSetDevice(trades->ctx->device));
    trades->grouping.segment = records;
    trades->grouping.blocks = blocks;
    ADR_HIP(apply_schedule_groups(trades));
    return ADR_OK;
}

int adr_trades_schedule_groups_info(const adr_trades* trades, int64_t* info) {
    if (!trades || !info) return fail(ADR_ERR_INVALID, "adr_trades_schedule_groups_info: null argument");
    const adr_trades::Grouping& G = trades->grouping;
    info[0] = G.found.n_groups; info[1] = G.found.n_grouped; info[2] = G.active ? 1 : 0;
    info[3] = G.used_groups; info[4] = G.used_trades; info[5] = G.segment > 0 ? G.segment : kScheduleSegment; info[6] = G.blocks;
    return ADR_OK;
}

int adr_schedule_groups_host(int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                             const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                             const double* flt_weight, const double* notional, const double* spread, const double* fix_sign,
                             const double* flt_sign, int32_t* group_of, double* cF, double* cX, int64_t* basis_fix_off,
                             int64_t* basis_flt_off, double* basis_fix_tp, double* basis_fix_pay, double* basis_flt_tp,
                             double* basis_flt_ts, double* basis_flt_te, double* basis_flt_alpha, double* basis_notional,
                             double* basis_spread) {
    if (n < 0 || (n > 0 && (!fix_off || !flt_off || !notional || !spread || !fix_sign || !flt_sign || !group_of || !cF || !cX)) ||
        !basis_fix_off || !basis_flt_off)
        return fail(ADR_ERR_INVALID, "adr_schedule_groups_host: bad count / null array");
    if (n > INT32_MAX) return fail(ADR_ERR_UNSUPPORTED, "adr_schedule_groups_host: more than 2^31 trades");
    for (int64_t t = 0; t < n; ++t)
        if (fix_off[t + 1] < fix_off[t] || flt_off[t + 1] < flt_off[t] || fix_off[0] != 0 || flt_off[0] != 0)
            return fail(ADR_ERR_INVALID, "adr_schedule_groups_host: offsets must start at 0 and be non-decreasing");
    std::vector<uint8_t> lagged_of(static_cast<size_t>(n), 0);
    R::flag_lagged(0, n, flt_off, flt_tp, flt_te, flt_alpha, flt_weight, lagged_of.data());
    std::vector<int32_t> eligible;           // the rule of the plain row table (route.cpp, trade_layout)
    for (int64_t t = 0; t < n; ++t)
        if (!lagged_of[static_cast<size_t>(t)] && fix_off[t + 1] - fix_off[t] <= adr::kRowSlots && flt_off[t + 1] - flt_off[t] <= adr::kRowSlots)
            eligible.push_back(static_cast<int32_t>(t));
    const adr::CsrHost csr{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, notional, spread, fix_sign, flt_sign};
    adr::ScheduleGroups F;
    adr::build_schedule_groups(csr, eligible.data(), static_cast<int64_t>(eligible.size()), F);
    std::copy(F.group_of.begin(), F.group_of.end(), group_of);
    std::copy(F.cF.begin(), F.cF.end(), cF);
    std::copy(F.cX.begin(), F.cX.end(), cX);
    std::copy(F.fix_off.begin(), F.fix_off.end(), basis_fix_off);
    std::copy(F.flt_off.begin(), F.flt_off.end(), basis_flt_off);
    auto give = [](const std::vector<double>& v, double* dst) { if (dst) std::copy(v.begin(), v.end(), dst); };
    give(F.fix_tp, basis_fix_tp); give(F.fix_pay, basis_fix_pay); give(F.flt_tp, basis_flt_tp); give(F.flt_ts, basis_flt_ts);
    give(F.flt_te, basis_flt_te); give(F.flt_alpha, basis_flt_alpha); give(F.notional, basis_notional); give(F.spread, basis_spread);
    return static_cast<int>(F.n_groups);
}

int64_t adr_trades_count(const adr_trades* t) { return t ? t->dev.n : 0; }

int64_t adr_trades_input_bytes(const adr_trades* t) {
    if (!t) return 0;
    return 16 * t->n_fix_flows + 32 * t->n_flt_flows + 40 * t->dev.n;
}

int adr_trades_upload(adr_ctx* ctx, int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp,
                      const double* fix_pay, const double* flt_tp, const double* flt_ts, const double* flt_te,
                      const double* flt_alpha, const double* notional, const double* spread, const double* fix_sign,
                      const double* flt_sign, adr_trades** out) {
    return adr_trades_upload_weighted(ctx, n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha,
                                      nullptr, notional, spread, fix_sign, flt_sign, out);
}

int adr_trades_upload_weighted(adr_ctx* ctx, int64_t n, const int64_t* fix_off, const int64_t* flt_off,
                               const double* fix_tp, const double* fix_pay, const double* flt_tp, const double* flt_ts,
                               const double* flt_te, const double* flt_alpha, const double* flt_weight,
                               const double* notional, const double* spread, const double* fix_sign,
                               const double* flt_sign, adr_trades** out) {
    if (!ctx || !out) return fail(ADR_ERR_INVALID, "adr_trades_upload: null ctx/out");
    *out = nullptr;
    if (n < 0) return fail(ADR_ERR_INVALID, "adr_trades_upload: negative trade count");
    if (n > 0 && (!fix_off || !flt_off || !notional || !spread || !fix_sign || !flt_sign))
        return fail(ADR_ERR_INVALID, "adr_trades_upload: null per-trade array");
    if (n > INT32_MAX) return fail(ADR_ERR_UNSUPPORTED, "adr_trades_upload: more than 2^31 trades in one batch");
    const int64_t n_fix = n ? fix_off[n] : 0, n_flt = n ? flt_off[n] : 0;
    if (n > 0 && (fix_off[0] != 0 || flt_off[0] != 0))
        return fail(ADR_ERR_INVALID, "adr_trades_upload: offsets must start at 0");

    // Validation: a single pass over the caller's arrays, cut into contiguous trade ranges for a pool of threads.
    const int n_threads = adr::pool_threads(n, 4096);
    auto parallel_ranges = [&](auto&& body) {          // body(range, first trade, one past the last trade); host_pool.hpp
        adr::parallel_ranges(n, n_threads, body);
    };
    // the offsets index the caller's arrays: check them before anything walks those arrays
    {
        std::vector<char> bad(static_cast<size_t>(n_threads), 0);
        parallel_ranges([&](int k, int64_t t0, int64_t t1) {
            for (int64_t t = t0; t < t1; ++t) {
                const int64_t mf = fix_off[t + 1] - fix_off[t], ml = flt_off[t + 1] - flt_off[t];
                if (mf < 0 || ml < 0 || mf > INT16_MAX || ml > INT16_MAX) { bad[static_cast<size_t>(k)] = 1; return; }
            }
        });
        for (char b : bad)
            if (b) return fail(ADR_ERR_INVALID, "adr_trades_upload: offsets must be non-decreasing, <= 32767 flows per leg");
    }
    if (n_fix > INT32_MAX || n_flt > INT32_MAX)
        return fail(ADR_ERR_UNSUPPORTED, "adr_trades_upload: more than 2^31 cash flows in one batch; shard the portfolio");
    if ((n_fix > 0 && (!fix_tp || !fix_pay)) || (n_flt > 0 && (!flt_tp || !flt_ts || !flt_te || !flt_alpha)))
        return fail(ADR_ERR_INVALID, "adr_trades_upload: null cash-flow array");

    // NaN / infinite inputs would only produce NaN outputs (every table index in the kernels is clamped), but a
    // batch that contains them is a caller error: say so here instead of returning a ladder of NaNs.  The same pass flags
    // the trades with payment lag or per-coupon notionals (route.hpp, flag_lagged).
    std::vector<uint8_t> lagged_of(static_cast<size_t>(n), 0);
    {
        std::vector<char> bad(static_cast<size_t>(n_threads), 0);       // 1: not finite, 2: bad sign
        parallel_ranges([&](int k, int64_t t0, int64_t t1) {
            char err = 0;
            auto finite = [](const double* a, int64_t lo, int64_t hi) {
                bool ok = true;
                for (int64_t i = lo; i < hi; ++i) ok &= std::isfinite(a[i]);
                return ok;
            };
            if (t1 > t0) {
                const int64_t f0 = fix_off[t0], f1 = fix_off[t1], l0 = flt_off[t0], l1 = flt_off[t1];
                if (!finite(fix_tp, f0, f1) || !finite(fix_pay, f0, f1) || !finite(flt_tp, l0, l1) || !finite(flt_ts, l0, l1) ||
                    !finite(flt_te, l0, l1) || !finite(flt_alpha, l0, l1) || (flt_weight && !finite(flt_weight, l0, l1)) ||
                    !finite(notional, t0, t1) || !finite(spread, t0, t1))
                    err = 1;
            }
            for (int64_t t = t0; t < t1 && !err; ++t)
                if (!(fix_sign[t] == 1.0 || fix_sign[t] == -1.0) || !(flt_sign[t] == 1.0 || flt_sign[t] == -1.0)) err = 2;
            if (!err) R::flag_lagged(t0, t1, flt_off, flt_tp, flt_te, flt_alpha, flt_weight, lagged_of.data());
            bad[static_cast<size_t>(k)] = err;
        });
        for (char b : bad)
            if (b == 1) return fail(ADR_ERR_INVALID, "adr_trades_upload: times, amounts, accruals, notionals and spreads must be finite");
        for (char b : bad)
            if (b == 2) return fail(ADR_ERR_INVALID, "adr_trades_upload: leg signs must be +1 or -1");
    }

    // which table or list every trade lands in, and the host side of those tables (route.cpp); they are gathered on the
    // device (trades_build.hip)
    R::TradeLayout L;
    if (const int rc = layout_trades("adr_trades_upload", n, fix_off, flt_off, flt_tp, flt_te, flt_alpha, flt_weight, ctx->n_cu, true, lagged_of, L))
        return rc;

    ADR_HIP(hipSetDevice(ctx->device));
    adr_trades* tr = new (std::nothrow) adr_trades();
    if (!tr) return fail(ADR_ERR_NOMEM, "adr_trades_upload: out of memory");
    tr->ctx = ctx;
    tr->n_fix_flows = n_fix;
    tr->n_flt_flows = n_flt;
    tr->counts = L.counts;
    {
        const auto it = std::find(lagged_of.begin(), lagged_of.end(), uint8_t(1));
        if (it != lagged_of.end()) tr->first_ratio = it - lagged_of.begin();
    }
    adr::DeviceOwner& mem = tr->mem;
    hipStream_t stream = ctx->stream;
    // (The host memory handed to `put` - the caller's arrays and the layout - outlives the asynchronous copies: it is kept
    // until the final synchronisation.  An empty array is null here, unlike in the schedule groups' tables.)
    const size_t nn = static_cast<size_t>(n), nf = static_cast<size_t>(n_fix), nl = static_cast<size_t>(n_flt);

    // the caller's arrays, once
    adr::CsrDev csr{};
    csr.n = n;
    csr.fix_off = mem.put_n(fix_off, nn ? nn + 1 : 0, stream, kBatchPad);
    csr.flt_off = mem.put_n(flt_off, nn ? nn + 1 : 0, stream, kBatchPad);
    csr.fix_tp = mem.put_n(fix_tp, nf, stream, kBatchPad);
    csr.fix_pay = mem.put_n(fix_pay, nf, stream, kBatchPad);
    csr.flt_tp = mem.put_n(flt_tp, nl, stream, kBatchPad);
    csr.flt_ts = mem.put_n(flt_ts, nl, stream, kBatchPad);
    csr.flt_te = mem.put_n(flt_te, nl, stream, kBatchPad);
    csr.flt_alpha = mem.put_n(flt_alpha, nl, stream, kBatchPad);
    csr.flt_weight = flt_weight ? mem.put_n(flt_weight, nl, stream, kBatchPad) : nullptr;
    csr.notional = mem.put_n(notional, nn, stream, kBatchPad);
    csr.spread = mem.put_n(spread, nn, stream, kBatchPad);
    csr.fix_sign = mem.put_n(fix_sign, nn, stream, kBatchPad);
    csr.flt_sign = mem.put_n(flt_sign, nn, stream, kBatchPad);

    tr->dev.n = n;
    tr->dev.any_ratio = L.any_lagged ? 1 : 0;
    {
        adr::TradeHeader* hdr = mem.array<adr::TradeHeader>(nn, kBatchPad);
        if (mem.ok() && n > 0) mem.note(adr::launch_build_headers(csr, hdr, stream));
        tr->dev.header = hdr;
    }
    tr->dev.fix_tp = csr.fix_tp; tr->dev.fix_pay = csr.fix_pay; tr->dev.flt_tp = csr.flt_tp; tr->dev.flt_ts = csr.flt_ts;
    tr->dev.flt_te = csr.flt_te; tr->dev.flt_alpha = csr.flt_alpha; tr->dev.flt_weight = csr.flt_weight;
    tr->dev.list = nullptr;
    tr->dev.n_list = n;

    // The row tables of the fast kernel (build_row_table).  The plain one lives in tr->dev itself; every other set starts
    // from a copy of tr->dev as it stands.
    const struct { int set; bool chained, lagged; } row_tables[] = {
        {R::S_ROWS, false, false},                      // plain table: one row per trade, sorted by coupon count
        {R::S_CHAINED, true, false},                    // longer trades as chains of 32-coupon rows
        {R::S_LAGGED, false, true},                     // payment-lag rows, one per trade (GAMMA on the packed layout)
        {R::S_LAGGED_CHAINED, true, true},              // ... chains of them (33-128 coupons)
    };
    for (const auto& rt : row_tables) {
        adr::TradesDev& dst = rt.set == R::S_ROWS ? tr->dev : tr->set[rt.set];
        if (rt.set != R::S_ROWS) dst = tr->dev;
        build_row_table(csr, rt.chained ? L.chain_trade[rt.set] : L.trades[rt.set], rt.chained ? &L.chain_first[rt.set] : nullptr,
                        rt.chained ? &L.chain_more[rt.set] : nullptr, rt.lagged, flt_weight != nullptr, mem, stream, dst);
    }
    tr->set[R::S_ROWS] = tr->dev;
    // the trade lists of the general / wide / tiled kernels; S_ALL: the identity
    for (int s = R::S_GENERAL; s <= R::S_ALL; ++s) {
        tr->set[s] = tr->dev;
        if (s != R::S_ALL) { tr->set[s].list = mem.put(L.trades[s], stream, kBatchPad); tr->set[s].n_list = static_cast<int64_t>(L.trades[s].size()); }
    }
    // per-wave scratch of the payment-lag variant: its special nodes' stash (read by the owning wave only: no pad)
    if (tr->counts.lag_scratch)
        tr->lag_scratch = static_cast<double*>(mem.alloc_zeroed(adr::fast_kernel_lag_scratch_bytes(tr->counts.lag_blocks), stream));
    // lite tables (kernels.hpp, LiteRowsDev): gathered on the device from their slots' trades and their rows' slot and piece
    for (int s : {R::S_LITE, R::S_LITE_LAG}) {
        constexpr int S = adr::kLiteSlots;
        adr::LiteRowsDev& lt = tr->lite[s];
        lt = L.lite[s];
        if (L.trades[s].empty()) continue;
        adr::LiteBuildDev lb{};
        const size_t n_rows = L.lite_row_slot[s].size(), n_slots = L.trades[s].size();
        lb.rows = static_cast<int64_t>(n_rows); lb.n_slots = static_cast<int64_t>(n_slots);
        lb.slot_trade = mem.put(L.trades[s], stream, kBatchPad);
        lb.row_slot = mem.put(L.lite_row_slot[s], stream, kBatchPad);
        lb.row_piece = mem.put(L.lite_row_piece[s], stream, kBatchPad);
        lb.tp_ts = mem.array<double>(n_rows * S * 2, kBatchPad);
        lb.al_xtp = mem.array<double>(n_rows * S * 2, kBatchPad);
        lb.xpay = mem.array<double>(n_rows * S, kBatchPad);
        lb.te_w = s == R::S_LITE_LAG ? mem.array<double>(n_rows * S * 2, kBatchPad) : nullptr;
        lb.slot = mem.array<adr::LiteTrade>(n_slots, kBatchPad);
        if (mem.ok()) mem.note(adr::launch_build_lite(csr, lb, stream));
        lt.tp_ts = lb.tp_ts; lt.al_xtp = lb.al_xtp; lt.xpay = lb.xpay; lt.te_w = lb.te_w; lt.slot = lb.slot;
    }
    // schedule groups among the trades of the plain row table: the host search runs while the device gathers the tables above
    // (apply_schedule_groups synchronises the stream before it builds its own)
    if (mem.ok() && !L.trades[R::S_ROWS].empty()) {
        const adr::CsrHost host{n, fix_off, flt_off, fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, notional, spread, fix_sign, flt_sign};
        adr::build_schedule_groups(host, L.trades[R::S_ROWS].data(), static_cast<int64_t>(L.trades[R::S_ROWS].size()), tr->grouping.found);
        if (tr->grouping.found.n_groups > 0) {
            tr->grouping.rows_order = L.trades[R::S_ROWS];
            tr->grouping.csr = csr;
            mem.note(apply_schedule_groups(tr));
        } else {
            tr->grouping.found = adr::ScheduleGroups();
        }
    }
    // the copies and the table builders run on the ctx's stream: the batch is usable once they are done
    mem.note(hipStreamSynchronize(stream));                  // (also on errors: the copies read the caller's arrays and `L`)
    if (!mem.ok()) {
        const hipError_t e = mem.error;
        adr_free_trades(tr);
        return fail_hip(e, "adr_trades_upload: copying trades");
    }
    *out = tr;
    return ADR_OK;
}

// ------------------------------------------------------------------------------------------- price
int adr_price_dev(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, uint32_t req_mask, double* pv_dev,
                  double* delta_dev, double* gamma_dev, double* agg_dev, void* stream_v) {
    if (!ctx || !curve || !trades) return fail(ADR_ERR_INVALID, "adr_price: null ctx/curve/trades");
    if (curve->ctx != ctx || trades->ctx != ctx)
        return fail(ADR_ERR_INVALID, "adr_price: curve/trades were uploaded through another ctx");
    const bool want_gamma = (req_mask & ADR_REQ_GAMMA) != 0;
    const bool want_delta = want_gamma || (req_mask & ADR_REQ_DELTA) != 0;
    if (want_gamma && !curve->dev.lc_lanes && !curve->dev.lcflat)
        return fail(ADR_ERR_INVALID, "adr_price: GAMMA requested but the curve was uploaded without hess");
    hipStream_t stream = stream_v ? static_cast<hipStream_t>(stream_v) : ctx->stream;
    const int P = curve->dev.P;
    const int64_t n = trades->dev.n;
    const size_t agg_bytes = sizeof(double) * (1 + P + static_cast<size_t>(P) * P);

    ADR_HIP(hipSetDevice(ctx->device));
    if (n == 0) {   // empty portfolio: the aggregate is all zeros, nothing else to write
        if (agg_dev) ADR_HIP(hipMemsetAsync(agg_dev, 0, agg_bytes, stream));
        return ADR_OK;
    }

    adr::OutputsDev o{};
    o.stamps = ctx->stamps;
    o.dump = ctx->dump;
    o.pv = (req_mask & ADR_REQ_VALUE) ? pv_dev : nullptr;
    o.delta = (req_mask & ADR_REQ_DELTA) ? delta_dev : nullptr;
    o.gamma = want_gamma ? gamma_dev : nullptr;
    o.lag_scratch = trades->lag_scratch;
    o.knot_partials = ctx->knot_partials;
    o.knot_overflow = ctx->knot_overflow;

    // The launch plan (route.hpp): which kernel family takes which of the batch's tables / lists.  It depends on the curve's
    // class, the batch's table sizes and the request only; the batch keeps the last one (a book is priced again and again on
    // scenario curves of one class).
    const bool per_trade = o.pv || o.delta || o.gamma;
    const std::shared_ptr<const R::Plan> held = trades->plan_for(curve->cls, want_delta, want_gamma, per_trade, agg_dev != nullptr, ctx->n_cu);
    const R::Plan& plan = *held;
    if (plan.error) return fail(ADR_ERR_INVALID, std::string("adr_price: ") + plan.error);

    const int stride = plan.wide ? adr::wide_partial_doubles(curve->dev.wide_nch) : adr::kAggStride;
    if (plan.tiled && agg_dev)   // tiles no launch covers (no GAMMA: the off-diagonal ones; PV alone: every delta tile) stay zero
        ADR_HIP(hipMemsetAsync(agg_dev, 0, agg_bytes, stream));
    const R::Launch *knot = nullptr, *knot_lag = nullptr;
    for (const R::Launch& L : plan.launches) {
        o.block_partials = agg_dev ? ctx->partials + static_cast<size_t>(L.first_block) * stride : nullptr;
        switch (L.family) {
            case R::F_LITE:
            case R::F_LITE_LAG: ADR_HIP(adr::launch_price_lite(curve->dev, trades->lite[L.set], o, want_delta, L.blocks, stream)); break;
            case R::F_FAST:
                if (L.set == R::S_ROWS && want_gamma && o.gamma && agg_dev && trades->grouping.active) {
                    // Schedule groups: the basis trades of every group into the batch's basis buffers,
                    // the members' ladders from them in a store pass, the fast kernel for the plain rows outside the groups.
                    // (With agg_dev only: such calls are serial on the ctx - include/adrates.h -, so nothing else is using
                    // the batch's basis buffers.)  The grouped trades' share of the aggregate goes to block records of the
                    // launch's range that no block wrote, slices of the groups in group order; the rest of them are zeroed.
                    const adr_trades::Grouping& G = trades->grouping;
                    const int per_cu = static_cast<int>(std::max<size_t>(1, std::min<size_t>(2, kLdsBudget / adr::fast_kernel_lds_bytes(curve->dev, true))));
                    const int waves = adr::fast_kernel_threads(false) / 64, groups = adr::fast_kernel_groups();
                    const int64_t cap = static_cast<int64_t>(ctx->n_cu) * per_cu;
                    adr::OutputsDev ob = o;
                    ob.pv = G.combine.b_pv; ob.delta = G.combine.b_delta; ob.gamma = G.combine.b_gamma; ob.block_partials = nullptr;
                    ADR_HIP(adr::launch_price_fast(curve->dev, G.basis, ob, true, true,
                                                   R::blocks_for((G.basis.n_rows + groups - 1) / groups, waves, cap), stream));
                    ADR_HIP(adr::launch_combine(G.combine, P, o.pv, o.delta, o.gamma, stream));
                    int prior = 0;
                    if (G.ungrouped.n_rows > 0) {
                        // (one record of the launch's range is kept free for the groups' share when there are two or more)
                        prior = std::min(std::max(1, L.blocks - 1), R::blocks_for((G.ungrouped.n_rows + groups - 1) / groups, waves, cap));
                        ADR_HIP(adr::launch_price_fast(curve->dev, G.ungrouped, o, want_delta, want_gamma, prior, stream));
                    }
                    ADR_HIP(adr::launch_group_aggregate(G.combine, P, o.block_partials, prior, L.blocks, stream));
                    break;
                }
                [[fallthrough]];
            case R::F_FAST_CHAINED:
            case R::F_FAST_LAG:
            case R::F_FAST_LAG_CHAINED: ADR_HIP(adr::launch_price_fast(curve->dev, trades->set[L.set], o, want_delta, want_gamma, L.blocks, stream)); break;
            case R::F_GENERAL: ADR_HIP(adr::launch_price_general(curve->dev, trades->set[L.set], o, want_delta, want_gamma, L.blocks, stream)); break;
            case R::F_WIDE: ADR_HIP(adr::launch_price_wide(curve->dev, trades->set[L.set], o, want_delta, want_gamma, L.blocks, stream)); break;
            case R::F_TILED: {
                // each launch writes its tile of the ladders; its partials are reduced into its tile of the aggregate
                adr::CurveDev cv = curve->dev;
                cv.tile_i = L.tile_i; cv.tile_j = L.tile_j;
                const size_t pair_tile = static_cast<size_t>(curve->dev.Kc) * 64 * adr::kGammaPerLane;
                if (cv.lc_lanes) cv.lc_lanes += static_cast<size_t>(adr::tile_pair(L.tile_i, L.tile_j)) * pair_tile;
                if (cv.lc_block_mask) cv.lc_block_mask += static_cast<size_t>(adr::tile_pair(L.tile_i, L.tile_j)) * curve->dev.Kc;
                ADR_HIP(adr::launch_price_general(cv, trades->set[L.set], o, want_delta, want_gamma, L.blocks, stream));
                if (agg_dev)
                    ADR_HIP(adr::launch_reduce_partials(o.block_partials, L.blocks, P, want_gamma, agg_dev, stream, L.tile_i, L.tile_j));
                break;
            }
            case R::F_KNOT: knot = &L; break;
            case R::F_KNOT_LAG: knot_lag = &L; break;
            default: return fail(ADR_ERR_INVALID, "adr_price: unknown kernel family in the launch plan");
        }
    }
    if (agg_dev && !plan.tiled) {
        if (plan.total_blocks == 0) ADR_HIP(hipMemsetAsync(agg_dev, 0, agg_bytes, stream));
        else if (plan.wide) ADR_HIP(adr::launch_reduce_wide(curve->dev, ctx->partials, plan.total_blocks, want_delta, want_gamma, agg_dev, stream));
        else ADR_HIP(adr::launch_reduce_partials(ctx->partials, plan.total_blocks, P, want_gamma, agg_dev, stream));
    }
    if (knot) {
        // aggregate-only request (agg and no per-trade output - Portfolio.compute's single ladder): the lite table's trades
        // are summed in KNOT space and projected once (kernels_lite.hip KNOT instantiations, kernels_knot.hip); the
        // projection ADDS to what the other families' reduction wrote above
        ADR_HIP(adr::launch_price_knot(curve->dev, trades->lite[knot->set], o, want_gamma, knot->blocks, stream));
        ADR_HIP(adr::launch_knot_project(curve->dev, ctx->knot_partials, knot->blocks, ctx->knot_reduced, want_delta, want_gamma, 1, nullptr, agg_dev, stream));
    }
    if (knot_lag) {
        // ... and the payment-lag rows' ratio nodes: pair bands per wave, pairs farther apart in the launch's overflow matrix
        const size_t kc = static_cast<size_t>(curve->dev.Kc);
        if (want_gamma) ADR_HIP(hipMemsetAsync(ctx->knot_overflow, 0, sizeof(double) * (kc * kc + 1), stream));   // (+ the "in use" flag)
        ADR_HIP(adr::launch_price_knot(curve->dev, trades->lite[knot_lag->set], o, want_gamma, knot_lag->blocks, stream));
        ADR_HIP(adr::launch_knot_project(curve->dev, ctx->knot_partials, knot_lag->blocks, ctx->knot_reduced, want_delta, want_gamma,
                                         adr::kKnotBand, ctx->knot_overflow, agg_dev, stream));
    }
    return ADR_OK;
}


int adr_price(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, uint32_t req_mask, double* pv,
              double* delta, double* gamma, double* agg) {
    if (!ctx || !curve || !trades) return fail(ADR_ERR_INVALID, "adr_price: null ctx/curve/trades");
    const int P = curve->dev.P;
    const size_t n = static_cast<size_t>(trades->dev.n);
    const size_t n_agg = 1 + P + static_cast<size_t>(P) * P;
    ADR_HIP(hipSetDevice(ctx->device));
    adr::DeviceOwner tmp;                     // the call's output arrays on the device
    double* d_pv = (pv && (req_mask & ADR_REQ_VALUE)) ? tmp.array<double>(n) : nullptr;
    double* d_delta = (delta && (req_mask & ADR_REQ_DELTA)) ? tmp.array<double>(n * P) : nullptr;
    double* d_gamma = (gamma && (req_mask & ADR_REQ_GAMMA)) ? tmp.array<double>(n * P * P) : nullptr;
    double* d_agg = agg ? tmp.array<double>(n_agg) : nullptr;
    if (!tmp.ok()) return fail_hip(tmp.release(), "adr_price: allocating outputs");
    const int rc = adr_price_dev(ctx, curve, trades, req_mask, d_pv, d_delta, d_gamma, d_agg, nullptr);
    if (rc != ADR_OK) { tmp.release(); return rc; }
    tmp.note(hipStreamSynchronize(ctx->stream));
    if (tmp.ok() && d_pv) tmp.note(hipMemcpy(pv, d_pv, n * sizeof(double), hipMemcpyDeviceToHost));
    if (tmp.ok() && d_delta) tmp.note(hipMemcpy(delta, d_delta, n * P * sizeof(double), hipMemcpyDeviceToHost));
    if (tmp.ok() && d_gamma) tmp.note(hipMemcpy(gamma, d_gamma, n * P * P * sizeof(double), hipMemcpyDeviceToHost));
    if (tmp.ok() && d_agg) tmp.note(hipMemcpy(agg, d_agg, n_agg * sizeof(double), hipMemcpyDeviceToHost));
    const hipError_t e = tmp.release();
    if (e != hipSuccess) return fail_hip(e, "adr_price: running kernels / copying results");
    return ADR_OK;
}

// ------------------------------------------------------------------------ cross-currency foreign leg, two curves
int adr_price_xccy_foreign_dev(adr_ctx* ctx, const adr_curve* foreign_curve, const adr_curve* xccy_curve, const adr_trades* legs,
                               uint32_t req_mask, double* pv_dev, double* delta_foreign_dev, double* delta_basis_dev,
                               double* agg_foreign_dev, double* agg_basis_dev, void* stream_v) {
    if (!ctx || !foreign_curve || !xccy_curve || !legs) return fail(ADR_ERR_INVALID, "adr_price_xccy_foreign: null ctx/curve/legs");
    if (foreign_curve->ctx != ctx || xccy_curve->ctx != ctx || legs->ctx != ctx)
        return fail(ADR_ERR_INVALID, "adr_price_xccy_foreign: curves/legs were uploaded through another ctx");
    if (req_mask & ADR_REQ_GAMMA)
        return fail(ADR_ERR_UNSUPPORTED, "adr_price_xccy_foreign: GAMMA takes the three-batch route (adr_trades_upload_weighted + adr_price)");
    const adr::CurveDev &cf = foreign_curve->dev, &cx = xccy_curve->dev;
    if (cf.T > 1 || cx.T > 1 || (cf.method == ADR_INTERP_LINEAR_FWD_RATES) != (cx.method == ADR_INTERP_LINEAR_FWD_RATES))
        return fail(ADR_ERR_UNSUPPORTED, "adr_price_xccy_foreign: curves of up to 32 pillars, both on LINEAR_FWD_RATES or neither");
    if (adr::lite_xc_kernel_lds_bytes(cf, cx) > kLdsBudget)
        return fail(ADR_ERR_UNSUPPORTED, "adr_price_xccy_foreign: the two curves' tables exceed the LDS of a CU");
    const int64_t n = legs->dev.n;
    hipStream_t stream = stream_v ? static_cast<hipStream_t>(stream_v) : ctx->stream;
    ADR_HIP(hipSetDevice(ctx->device));
    const int Pf = cf.P, Px = cx.P;
    const size_t agg_f_bytes = sizeof(double) * (1 + Pf + static_cast<size_t>(Pf) * Pf), agg_x_bytes = sizeof(double) * (1 + Px + static_cast<size_t>(Px) * Px);
    if (n == 0) {
        if (agg_foreign_dev) ADR_HIP(hipMemsetAsync(agg_foreign_dev, 0, agg_f_bytes, stream));
        if (agg_basis_dev) ADR_HIP(hipMemsetAsync(agg_basis_dev, 0, agg_x_bytes, stream));
        return ADR_OK;
    }
    // every leg must sit in the lite kernel's payment-lag rows (accrual end != payment time on some coupon, <= 390 coupons)
    const adr::LiteRowsDev& rows = legs->lite[R::S_LITE_LAG];
    if (legs->lite[R::S_LITE].n_units > 0 || legs->counts.n_nonlite_b > 0 || rows.n_units == 0)
        return fail(ADR_ERR_UNSUPPORTED, "adr_price_xccy_foreign: a leg is outside the payment-lag row table (more than 390 coupons, "
                                         "or no coupon whose accrual end differs from its payment time)");
    // one block per CU: its registers leave room for the block's own three waves per SIMD
    const int blocks = R::blocks_for(rows.n_units, adr::lite_xc_kernel_threads() / 64, static_cast<int64_t>(ctx->n_cu));
    if (2 * blocks > ctx->max_blocks) return fail(ADR_ERR_INVALID, "adr_price_xccy_foreign: grid exceeds scratch");
    const bool want_agg = agg_foreign_dev || agg_basis_dev;
    adr::OutputsDev o{};
    o.pv = (req_mask & ADR_REQ_VALUE) ? pv_dev : nullptr;
    o.delta = (req_mask & ADR_REQ_DELTA) ? delta_foreign_dev : nullptr;
    o.delta2 = (req_mask & ADR_REQ_DELTA) ? delta_basis_dev : nullptr;
    o.block_partials = want_agg ? ctx->partials : nullptr;
    o.block_partials2 = want_agg ? ctx->partials + static_cast<size_t>(blocks) * adr::kAggStride : nullptr;
    ADR_HIP(adr::launch_price_lite_xc(cf, cx, rows, o, blocks, stream));
    // (the kernel is built with DELTA only, so its block records always carry the delta sums: a request without DELTA drops
    // them in the reduction, which writes +0.0 there as adr_price does for a block that is not asked for)
    const bool has_delta = (req_mask & ADR_REQ_DELTA) != 0;
    if (agg_foreign_dev) ADR_HIP(adr::launch_reduce_partials(o.block_partials, blocks, Pf, false, agg_foreign_dev, stream, 0, 0, has_delta));
    if (agg_basis_dev) ADR_HIP(adr::launch_reduce_partials(o.block_partials2, blocks, Px, false, agg_basis_dev, stream, 0, 0, has_delta));
    return ADR_OK;
}

int adr_price_xccy_foreign(adr_ctx* ctx, const adr_curve* foreign_curve, const adr_curve* xccy_curve, const adr_trades* legs,
                           uint32_t req_mask, double* pv, double* delta_foreign, double* delta_basis, double* agg_foreign,
                           double* agg_basis) {
    if (!ctx || !foreign_curve || !xccy_curve || !legs) return fail(ADR_ERR_INVALID, "adr_price_xccy_foreign: null ctx/curve/legs");
    const size_t n = static_cast<size_t>(legs->dev.n), Pf = foreign_curve->dev.P, Px = xccy_curve->dev.P;
    ADR_HIP(hipSetDevice(ctx->device));
    adr::DeviceOwner tmp;                     // the call's output arrays on the device
    double* d_pv = (pv && (req_mask & ADR_REQ_VALUE)) ? tmp.array<double>(n) : nullptr;
    double* d_f = (delta_foreign && (req_mask & ADR_REQ_DELTA)) ? tmp.array<double>(n * Pf) : nullptr;
    double* d_x = (delta_basis && (req_mask & ADR_REQ_DELTA)) ? tmp.array<double>(n * Px) : nullptr;
    double* d_af = agg_foreign ? tmp.array<double>(1 + Pf + Pf * Pf) : nullptr;
    double* d_ax = agg_basis ? tmp.array<double>(1 + Px + Px * Px) : nullptr;
    if (!tmp.ok()) return fail_hip(tmp.release(), "adr_price_xccy_foreign: allocating outputs");
    const int rc = adr_price_xccy_foreign_dev(ctx, foreign_curve, xccy_curve, legs, req_mask, d_pv, d_f, d_x, d_af, d_ax, nullptr);
    if (rc != ADR_OK) { tmp.release(); return rc; }
    tmp.note(hipStreamSynchronize(ctx->stream));
    auto back = [&](double* dst, double* src, size_t count) { if (tmp.ok() && src) tmp.note(hipMemcpy(dst, src, count * sizeof(double), hipMemcpyDeviceToHost)); };
    back(pv, d_pv, n); back(delta_foreign, d_f, n * Pf); back(delta_basis, d_x, n * Px);
    back(agg_foreign, d_af, 1 + Pf + Pf * Pf); back(agg_basis, d_ax, 1 + Px + Px * Px);
    const hipError_t e = tmp.release();
    if (e != hipSuccess) return fail_hip(e, "adr_price_xccy_foreign: running the kernel / copying results");
    return ADR_OK;
}

// ---------------------------------------------------------------------------------------- launch plan, host side
int adr_route_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac, const double* hess,
                   uint32_t curve_flags, int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* flt_tp,
                   const double* flt_te, const double* flt_alpha, const double* flt_weight, uint32_t req_mask, int per_trade,
                   int aggregate, int n_cu, int32_t* cover, int32_t* launches, int max_launches) {
    if (n < 0 || (n > 0 && (!fix_off || !flt_off || !cover)) || !launches || max_launches < 1 || n_cu < 1)
        return fail(ADR_ERR_INVALID, "adr_route_host: bad argument");
    adr::CurveTables t;
    const std::string err = adr::build_curve_tables(K, P, times, dfs, jac, hess, t);
    if (!err.empty()) return fail(ADR_ERR_INVALID, "adr_route_host: " + err);
    const R::CurveClass cls = R::curve_class(t, interp_method, (curve_flags & ADR_CURVE_PILLAR_TILES) != 0);
    if ((req_mask & ADR_REQ_GAMMA) && !t.has_hess) return fail(ADR_ERR_INVALID, "adr_route_host: GAMMA requested but hess is null");
    std::vector<uint8_t> lagged_of;
    R::TradeLayout L;
    if (const int rc = layout_trades("adr_route_host", n, fix_off, flt_off, flt_tp, flt_te, flt_alpha, flt_weight, n_cu, false, lagged_of, L))
        return rc;
    const bool want_gamma = (req_mask & ADR_REQ_GAMMA) != 0, want_delta = want_gamma || (req_mask & ADR_REQ_DELTA) != 0;
    const R::Plan plan = R::make_plan(cls, L.counts, want_delta, want_gamma, per_trade != 0, aggregate != 0, n_cu);
    if (plan.error) return fail(ADR_ERR_INVALID, std::string("adr_route_host: ") + plan.error);
    // who is covered how often: the tile launches of one pass count once
    for (int64_t i = 0; i < n; ++i) cover[i] = 0;
    int n_out = 0;
    for (const R::Launch& Ln : plan.launches) {
        if (n_out < max_launches) {
            int32_t* row = launches + 4 * n_out;
            row[0] = Ln.family; row[1] = Ln.set; row[2] = static_cast<int32_t>(std::min<int64_t>(Ln.items, INT32_MAX)); row[3] = Ln.blocks;
        }
        ++n_out;
        if (Ln.family == R::F_TILED && !(Ln.tile_i == 0 && Ln.tile_j == 0)) continue;
        if (Ln.set == R::S_ALL) for (int64_t i = 0; i < n; ++i) ++cover[i];
        for (int32_t tr : L.trades[Ln.set]) if (tr >= 0) ++cover[tr];        // (-1: an empty slot of a lite table)
    }
    return n_out;
}

// ---------------------------------------------------------------------------------------- multi-GPU
int adr_allreduce_agg(adr_ctx* ctx, void* rccl_comm, double* agg_dev, int count, void* stream_v) {
    if (!ctx || !rccl_comm || !agg_dev || count <= 0) return fail(ADR_ERR_INVALID, "adr_allreduce_agg: bad argument");
    hipStream_t stream = stream_v ? static_cast<hipStream_t>(stream_v) : ctx->stream;
    ncclResult_t r = ncclAllReduce(agg_dev, agg_dev, static_cast<size_t>(count), ncclDouble, ncclSum,
                                   static_cast<ncclComm_t>(rccl_comm), stream);
    if (r != ncclSuccess) return fail(ADR_ERR_RCCL, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    return ADR_OK;
}

int adr_rccl_unique_id(void* id_out) {
    if (!id_out) return fail(ADR_ERR_INVALID, "adr_rccl_unique_id: null output");
    static_assert(sizeof(ncclUniqueId) == ADR_RCCL_ID_BYTES, "ADR_RCCL_ID_BYTES must equal sizeof(ncclUniqueId)");
    ncclUniqueId id;
    const ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(ADR_ERR_RCCL, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(id_out, &id, sizeof id);
    return ADR_OK;
}

int adr_rccl_comm_init(adr_ctx* ctx, const void* id, int n_ranks, int rank, void** comm_out) {
    if (!ctx || !id || !comm_out || n_ranks < 1 || rank < 0 || rank >= n_ranks)
        return fail(ADR_ERR_INVALID, "adr_rccl_comm_init: bad argument");
    *comm_out = nullptr;
    ADR_HIP(hipSetDevice(ctx->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof uid);
    ncclComm_t comm = nullptr;
    const ncclResult_t r = ncclCommInitRank(&comm, n_ranks, uid, rank);
    if (r != ncclSuccess) return fail(ADR_ERR_RCCL, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
    *comm_out = comm;
    return ADR_OK;
}

void adr_rccl_comm_destroy(void* rccl_comm) {
    if (rccl_comm) ncclCommDestroy(static_cast<ncclComm_t>(rccl_comm));
}

}  // extern "C"
