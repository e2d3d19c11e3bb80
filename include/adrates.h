/*
 * adrates.h - C-ABI of the MI355X-native OIS PV / delta / gamma path.
 *
 * The reference (ludcode/ADRates, "Cavour") is pure Python + JAX and has no FFI
 * of its own; the boundary this library replaces is the internal pure-function
 * seam of its valuation engine:
 *
 *   curve cache dict {times, dfs, jac, hess}   cavour/market/position/engine.py:2362-2412
 *   _price_fixed_leg_jax(dfs, times, interp, payment_times, payments, ...)     :2414-2448
 *   _float_leg_jax(dfs, times, interp, payment_times, start_times, end_times,
 *                  pay_alphas, spreads, notionals, ...)                         :2639-2728
 *   grad / hessian + chain rule to the pillar ladders                 :2541-2576, 2899-2934
 *   Portfolio.compute's running sums            cavour/market/portfolio/portfolio.py:39-66
 *
 * Conventions
 *   - every function returns 0 on success or a negative adr_status; the message
 *     for the calling thread's last failure is adr_last_error();
 *   - all arithmetic is IEEE float64; indices are int32/int64;
 *   - plain pointers and sizes only; "host" pointers are ordinary process memory,
 *     "_dev" pointers are HIP device memory of the ctx's GPU (e.g. a torch tensor's
 *     data_ptr);
 *   - a ctx is bound to one GPU and is not thread-safe; use one ctx per GPU/process;
 *   - there is no CPU fallback: adr_init fails when no HIP device is usable.
 */
#ifndef ADRATES_H
#define ADRATES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct adr_ctx adr_ctx;
typedef struct adr_curve adr_curve;
typedef struct adr_trades adr_trades;
typedef struct adr_curve_plan adr_curve_plan;
typedef struct adr_curve_set adr_curve_set;

typedef enum adr_status {
    ADR_OK = 0,
    ADR_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, unsorted times ...) */
    ADR_ERR_UNSUPPORTED = -2, /* interpolation method / pillar count outside what the kernels implement */
    ADR_ERR_HIP = -3,         /* a HIP runtime call failed; text has hipGetErrorString */
    ADR_ERR_NOMEM = -4,
    ADR_ERR_RCCL = -5
} adr_status;

/* Interpolation methods: values of the reference's InterpTypes enum
 * (cavour/utils/global_types.py:76-84) accepted by simple_interpolate
 * (cavour/market/curves/interpolator_ad.py:227-235). */
#define ADR_INTERP_FLAT_FWD_RATES 1
#define ADR_INTERP_LINEAR_FWD_RATES 2
#define ADR_INTERP_LINEAR_ZERO_RATES 4

/* Request mask bits: RequestTypes.VALUE / DELTA / GAMMA (cavour/utils/global_types.py:69-74). */
#define ADR_REQ_VALUE 1u
#define ADR_REQ_DELTA 2u
#define ADR_REQ_GAMMA 4u

/* Largest pillar count of an uploaded curve (the reference has no limit, cavour/market/position/engine.py:2388-2389); larger
 * curves are refused with ADR_ERR_UNSUPPORTED, and so is one whose knot tables do not fit the 160 KiB LDS of a CU next to two
 * 32-pillar tiles of its Jacobian.  Up to 32 pillars: the fast / lite kernels; 33-64: one launch for the whole ladder (wide
 * layout); 65-256: 32-pillar tiles, one launch per tile pair.  Results do not depend on the pillar count's parity or on which
 * kernel family a curve is routed to (DESIGN.md section 5 describes the routes and their measured rates).  The LDS check binds
 * long before 256 pillars on realistic curves (about 12 bytes per knot and 536 per reachable knot): validated against the C
 * oracle are a curve of 155 pillars with a weekly short end (K = 2 021 knots, the largest such curve accepted) and one of 256
 * single-period pillars (K = 257).
 * adr_curve_plan_create (the device curve builder) takes up to ADR_MAX_PLAN_PILLARS. */
#define ADR_MAX_PILLARS 256
#define ADR_MAX_PLAN_PILLARS 64

/* Flags of adr_curve_upload_ex. */
#define ADR_CURVE_PILLAR_TILES 1u   /* curves of 33-64 pillars: price on 32-pillar tiles (one launch per tile pair) even when
                                       the single-launch layout fits the LDS; same results to rounding (diagnostics, A/B) */

int adr_version(void);
const char* adr_last_error(void);

/* One context per GPU: selects the device, creates the library's own stream and scratch. */
int adr_init(int device_ordinal, adr_ctx** out);
void adr_free_ctx(adr_ctx* ctx);
/* Number of HIP devices visible to the process (0 when none; never fails). */
int adr_device_count(void);

/*
 * Curve tables, replacing the reference's per-Engine cache dict
 * (engine.py:2405-2411): knot times [K] (non-decreasing, duplicates allowed and
 * meaningful), knot discount factors [K], jac = d dfs / d par-rates [K*P]
 * row-major, hess = d2 dfs / d par-rates2 [K*P*P] row-major (may be NULL when
 * gamma will never be requested).  The first knot must be the value-time point
 * the reference's grids start with (t = 0, discount factor 1, zero jac row): the
 * reference prices relative to D(0) (engine.py:2426-2435) and the kernels rely on
 * D(0) = 1 instead of dividing.  The library converts the tables to log space,
 * keeps only the knots a query can reference and uploads them.
 */
int adr_curve_upload(adr_ctx* ctx, int interp_method, int K, int P,
                     const double* times, const double* dfs,
                     const double* jac, const double* hess,
                     adr_curve** out);
/* The same with explicit layout flags (ADR_CURVE_*); adr_curve_upload is flags = 0. */
int adr_curve_upload_ex(adr_ctx* ctx, int interp_method, int K, int P,
                        const double* times, const double* dfs,
                        const double* jac, const double* hess,
                        uint32_t flags, adr_curve** out);
void adr_free_curve(adr_curve* curve);
int adr_curve_pillars(const adr_curve* curve);

/*
 * Host-side half of adr_curve_upload, exposed so the table construction can be
 * checked without a GPU: writes, for the Kc knots a query can reach,
 *   knot_index[Kc]  index into the caller's K knots,
 *   log_df[Kc]      ln dfs,
 *   lj[Kc*P]        d ln df_k / d r_p,
 *   lc[Kc*P*P]      d2 ln df_k / d r_p d r_q   (skipped when hess or lc is NULL).
 * Call with all outputs NULL to get Kc.  Returns Kc (>= 0) or a negative status.
 */
int adr_curve_tables_host(int K, int P, const double* times, const double* dfs,
                          const double* jac, const double* hess,
                          int32_t* knot_index, double* log_df, double* lj, double* lc);

/*
 * Diagnostic twin of adr_curve_tables_host: how the fast kernels would lay this curve out in LDS.
 * info[16] = { packed layout usable (0/1), core pillars Pc, core pairs Ec, packed entries Eu,
 *              entries per lane, core-table rows, short-end (mini) knots, LDS bytes of the gamma kernel,
 *              LDS bytes of the general kernel's variant with resident convexity rows (0: none), that variant fits (0/1),
 *              core slots per lane, hub layout found (0/1: the exact kernel variants; 0 = the universal ones),
 *              wide layout (33-64 pillars): 128-entry chunks per row of the packed triangle (7 / 10 / 17; 0: none),
 *              LDS bytes of the wide gamma kernel, the most chunks any knot's convexity row is read in,
 *              LDS bytes of the general kernel's tables that adr_curve_upload checks against the 160 KiB of a CU }.
 * Returns 0 or a negative status.  No GPU needed.
 */
int adr_curve_layout_host(int K, int P, const double* times, const double* dfs,
                          const double* jac, const double* hess, int64_t* info);

/*
 * Book compilers, host side (multi-threaded, no GPU): the coupon schedules of many swap legs at once, and the foreign-leg
 * batches of a cross-currency book.  They replace the per-swap Python the reference runs before its leg functions:
 * Schedule._generate (cavour/utils/schedule.py:163-270) + Calendar.adjust / add_business_days
 * (cavour/utils/calendar.py:139-253) + SwapFloatLeg.generate_payment_dts (cavour/trades/rates/swap_float_leg.py:130-186),
 * and the coupon loop of Engine._compute_xccy (cavour/market/position/engine.py:1486-1578, 1640-1712).
 *
 * Dates are Excel serials (Date.excel_dt(), >= 1-Mar-1900).  Conventions covered: BACKWARD date generation without
 * end-of-month rolling, the WEEKEND calendar (weekend_calendar 0: NONE), bd_type = BusDayAdjustTypes value (1 NONE,
 * 2 FOLLOWING, 3 MODIFIED_FOLLOWING, 4 PRECEDING, 5 MODIFIED_PRECEDING), payment lags in business days, day counts with a
 * fixed denominator.  adr_leg_counts_host: coupons per leg.  adr_leg_times_host: with off = the exclusive prefix sums of
 * those counts ([n + 1]), payment / accrual start / accrual end times as year fractions from value_serial (payment times on
 * payment_denominator when > 0, else on the leg's own), accrual fractions, and plain[i] = 1 when the leg's dates are
 * strictly increasing (0: the reference's schedule de-duplication applies - the entries are then not its schedule and the
 * caller takes the object route for that leg).
 */
int adr_leg_counts_host(int64_t n, const int64_t* eff, const int64_t* term, const int64_t* months_per_period,
                        int64_t* n_coupons);
int adr_leg_times_host(int64_t n, const int64_t* eff, const int64_t* term, const int64_t* months_per_period,
                       const int64_t* payment_lag, int bd_type, int weekend_calendar, const double* denominator,
                       int64_t value_serial, double payment_denominator, const int64_t* off, double* tp, double* ts,
                       double* te, double* alpha, uint8_t* plain);
/*
 * Foreign leg of n cross-currency basis swaps (CSR for_off over the coupons: payment times on the XCCY curve's day count,
 * accrual start / end times, accrual fractions) given the discount factors the device returned for them (adr_curve_df):
 * df_x [m + 1] = D_x at the m payment times, then at the value time; df_f [2 m] = D_f at the m accrual starts, then at the m
 * accrual ends: (1) the rate-ladder batch - every live accruing coupon
 * with its discount factor as notional multiplier (adr_trades_upload_weighted's flt_weight) -, (2) the fixed flows
 * N (fwd + spread) alpha at tp > 0 followed by the notional exchanges (exch_t [n][2] effective / maturity times, exch_on [n])
 * at t > 0, and (3) pv_const [n] (in: the domestic constants; out: + flows dated at the value time, in domestic currency).
 * Output arrays are sized by the caller for every coupon (rates_*: for_off[n]; flows_*: for_off[n] + 2 n); the offsets
 * ([n + 1]) say what was filled.
 */
/* The notional exchanges of n legs (exch_t [n][2]: effective / maturity times; on [n]): flows -N, +N at t > 0 as CSR arrays
 * (off [n + 1]; flow_tp / flow_pay sized 2 n), flows dated AT the value time as pv_const [n] = sum sign * amount / scale. */
int adr_exchange_flows_host(int64_t n, const double* exch_t, const double* notional, const uint8_t* on, const double* sign,
                            double scale, int64_t* off, double* flow_tp, double* flow_pay, double* pv_const);
int adr_xccy_assemble_host(int64_t n, const int64_t* for_off, const double* tp_x, const double* ts, const double* te,
                           const double* alpha, const double* df_x, const double* df_f, const double* for_n,
                           const double* for_spread, const double* for_sign, double spot, const double* exch_t,
                           const uint8_t* exch_on, int64_t* rates_off, double* rates_ts, double* rates_te,
                           double* rates_alpha, double* rates_weight, int64_t* flows_off, double* flows_tp,
                           double* flows_pay, double* pv_const);

/*
 * Curve builder on the device, for batches of par-rate scenarios on one knot grid.  It replaces
 * Engine.build_curve_ad (engine.py:2246-2360: the lax.scan d = (1 - r PV01_prev) / (1 + r acc)) and the
 * jacrev / hessian of Engine._cached_curve (engine.py:2388-2389) for the case the reference handles by
 * rebuilding a Model per shock (Model.scenario, cavour/models/models.py:507-557): the par rates change,
 * the schedules - hence the knot grid - do not.
 *
 * A plan holds what does not depend on the rates: the scan description of the K sorted bootstrap points
 * (engine.py:2283-2334) -
 *   times[K]     knot times (as for adr_curve_upload),
 *   acc[K]       accrual fraction of the coupon period ending at the knot (0 for the t = 0 point),
 *   pillar[K]    index of the calibration swap whose par rate the knot uses,
 *   prev_idx[K]  knot whose PV01 the knot builds on (first sorted point with the previous coupon's
 *                round(t, 2) key), -1 for a swap's first period,
 * and the table layout, taken from the base curve (base_dfs/base_jac/base_hess as for adr_curve_upload;
 * base_hess NULL = no gamma for any curve of the plan).  Curves built from a plan point into it: free
 * the sets before the plan.
 */
int adr_curve_plan_create(adr_ctx* ctx, int interp_method, int K, int P,
                          const double* times, const double* acc,
                          const int32_t* pillar, const int32_t* prev_idx,
                          const double* base_dfs, const double* base_jac, const double* base_hess,
                          adr_curve_plan** out);
void adr_free_curve_plan(adr_curve_plan* plan);

/*
 * Bootstrap n_scen curves (rates: host array [n_scen * P] of par rates, decimal) with their first and -
 * when the plan has hess - second par-rate derivatives on the GPU and convert them to the kernels' tables.
 * Blocks until the curves are ready.  adr_curve_set_get returns a curve owned by the set (do not free it)
 * that adr_price / adr_price_dev accept like an uploaded one.
 */
int adr_curve_set_build(adr_ctx* ctx, const adr_curve_plan* plan, int n_scen, const double* rates,
                        adr_curve_set** out);
int adr_curve_set_size(const adr_curve_set* set);
const adr_curve* adr_curve_set_get(const adr_curve_set* set, int i);
/* Copy scenario i's dense arrays back (any pointer may be NULL): dfs[K], jac[K*P], hess[K*P*P] - the
 * contents of the reference's cache dict for that scenario. */
int adr_curve_set_download(const adr_curve_set* set, int i, double* dfs, double* jac, double* hess);
void adr_free_curve_set(adr_curve_set* set);

/*
 * A batch of OIS trades in CSR form - the per-trade arrays the reference engine
 * extracts from the leg objects (engine.py:2519-2527 fixed, :2858-2877 float):
 *   fix_off/flt_off [n+1]  offsets into the cash-flow arrays (fix_off[0] = flt_off[0] = 0)
 *   fix_tp, fix_pay        fixed payment times (years from the value date) and amounts
 *   flt_tp/ts/te/alpha     float payment, accrual-start, accrual-end times and accrual fractions
 *   notional, spread       per trade (float-leg notional and spread)
 *   fix_sign, flt_sign     +1 receive / -1 pay, per trade
 * Value time is 0 and both principals are 0, as for every OIS the reference builds
 * (cavour/trades/rates/ois.py:149, swap_float_leg.py:106).
 * The arrays are validated on the host (a thread per contiguous trade range) and classified there (route.cpp,
 * trade_layout), copied to the device once, and the kernels' padded row tables are gathered from them ON THE DEVICE (trades_build.hip):
 * about 40 ms per million benchmark trades.  Blocks until the batch is usable; may be called from several
 * host threads on one ctx (it touches no shared state of the ctx but its stream).
 */
int adr_trades_upload(adr_ctx* ctx, int64_t n_trades,
                      const int64_t* fix_off, const int64_t* flt_off,
                      const double* fix_tp, const double* fix_pay,
                      const double* flt_tp, const double* flt_ts,
                      const double* flt_te, const double* flt_alpha,
                      const double* notional, const double* spread,
                      const double* fix_sign, const double* flt_sign,
                      adr_trades** out);
/*
 * The same with a weight per float coupon (flt_weight[sum n_flt], NULL = all 1) that multiplies the trade's
 * notional for that coupon.  It carries the discount factor of the *other* curve when a float leg is
 * discounted on one curve and projected on another - the foreign leg of a cross-currency swap, where the
 * reference calls _float_leg_jax with disc != index curve (engine.py:1640-1712): holding the XCCY curve fixed,
 * the sensitivities to the foreign OIS rates are those of sum_j w_j N D(ts_j)/D(te_j) with w_j = D_x(tp_j).
 * Trades with a weight != 1 are priced like payment-lag trades: the payment-lag rows of the lite kernel (PV / DELTA),
 * the payment-lag variant of the fast kernel (GAMMA, curves with the packed layout), the general kernel otherwise.
 */
int adr_trades_upload_weighted(adr_ctx* ctx, int64_t n_trades,
                               const int64_t* fix_off, const int64_t* flt_off,
                               const double* fix_tp, const double* fix_pay,
                               const double* flt_tp, const double* flt_ts,
                               const double* flt_te, const double* flt_alpha,
                               const double* flt_weight,
                               const double* notional, const double* spread,
                               const double* fix_sign, const double* flt_sign,
                               adr_trades** out);
void adr_free_trades(adr_trades* trades);
int64_t adr_trades_count(const adr_trades* trades);
/* Bytes of trade input one pricing pass has to read (SURVEY.md section 8(d):
 * 16 per fixed flow + 32 per float flow + 40 per trade). */
int64_t adr_trades_input_bytes(const adr_trades* trades);

/*
 * Schedule groups.  A trade's [pv, delta, gamma] is linear in its cash amounts, and everything
 * non-linear depends on its node times only; seen from the value date, the swaps of one maturity date and roll convention
 * share their remaining schedule.  adr_trades_upload finds, among the trades of the plain one-row table (no payment lag, no
 * weights, at most 32 coupons per leg), the groups whose coupon counts, times, accrual fractions and spread agree bit for bit
 * and whose fixed payments are proportional to 16 ulp of the last payment (a trade whose last payment is 0 joins only with a
 * fixed leg of zeros; a trade that fails the test stays ungrouped).  A pricing call then prices TWO basis trades per group -
 * the float leg per unit notional, the fixed leg per unit of its last payment - and forms the members' ladders as
 *   out[t] = cF BF[g] + cX BX[g],   cF = flt_sign notional,   cX = fix_sign fix_pay[last]
 * in a store pass; the plain-row trades outside the groups take the fast kernel as before.  Nothing in the grouping reads
 * notionals, coupon levels or signs: flipping a batch's signs negates its results exactly, doubling its amounts doubles them.
 *
 * adr_price_dev takes this route only for requests with GAMMA and a per-trade gamma pointer AND agg_dev != NULL: the basis
 * ladders live in buffers owned by the BATCH, and only aggregate-producing calls are serial on a ctx (stream rule 1 of
 * adr_price_dev) - calls without agg_dev may run concurrently on one batch and keep the direct route.  Results of the two
 * routes agree to rounding (about 1e-12 of the ladder's scale), not bit for bit.
 *
 * adr_trades_set_schedule_groups: AUTO (the default) uses the groups of at least 64 trades when the batch has at least 32768
 * trades in such groups; OFF never; FORCE every group of two or more trades whatever the batch size.
 * adr_trades_set_schedule_segment: records one wavefront of the store pass writes (0 = the default) and the size of its
 * grid (blocks = 0, the default: one wavefront per segment; else a persistent grid of that many 4-wave blocks walks the
 * segments) - the knobs DESIGN.md section 22 measures.  Both rebuild the
 * batch's device tables: they allocate and synchronise, and must not run while a pricing call on the batch is in flight or
 * between the capture and the last replay of a graph that prices it.
 * adr_trades_schedule_groups_info: info[7] = {groups of two or more found, trades in them, route active (0 / 1), groups in
 * use, trades in them, segment length, persistent blocks}.
 */
#define ADR_SCHEDULE_GROUPS_AUTO 0
#define ADR_SCHEDULE_GROUPS_OFF 1
#define ADR_SCHEDULE_GROUPS_FORCE 2
int adr_trades_set_schedule_groups(adr_trades* trades, int mode);
int adr_trades_set_schedule_segment(adr_trades* trades, int records, int blocks);
int adr_trades_schedule_groups_info(const adr_trades* trades, int64_t* info);
/*
 * The grouping alone, on the host (no GPU needed), for a batch given as the arrays of adr_trades_upload_weighted:
 * group_of[n] (-1: ungrouped; groups are numbered by their lowest trade), cF[n], cX[n] (0 for ungrouped trades) and the
 * basis trades as a CSR batch of 2 G pseudo-trades - 2g: the float leg of group g with notional 1 at the group's spread and
 * no fixed flows, 2g + 1: its fixed leg x^ with no float coupons and notional 0; all signs +1.  The caller sizes the basis
 * arrays for the worst case: basis_fix_off / basis_flt_off [n + 1], basis_notional / basis_spread [n], the fixed arrays
 * [fix_off[n]], the float arrays [flt_off[n]].  Returns G (every group of two or more trades) or a negative status.
 */
int adr_schedule_groups_host(int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                             const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                             const double* flt_weight, const double* notional, const double* spread, const double* fix_sign,
                             const double* flt_sign, int32_t* group_of, double* cF, double* cX, int64_t* basis_fix_off,
                             int64_t* basis_flt_off, double* basis_fix_tp, double* basis_fix_pay, double* basis_flt_tp,
                             double* basis_flt_ts, double* basis_flt_te, double* basis_flt_alpha, double* basis_notional,
                             double* basis_spread);

/*
 * Price the batch: per-trade PV [n], delta ladder [n*P] and gamma [n*P*P]
 * (row-major, full symmetric matrix), units as the reference: delta per 1 bp
 * (x1e-4), gamma per bp^2 (x1e-8).  Any output may be NULL; req_mask says what
 * to compute.  agg (optional) receives the portfolio sums laid out as
 * [pv, delta[P], gamma[P*P]] = 1 + P + P*P doubles - what Portfolio.compute
 * returns.  Whatever req_mask says, agg[0] holds the book's PV; the delta block
 * holds the book's delta when DELTA or GAMMA is requested, the gamma block its
 * gamma with GAMMA; a block not computed is zeros.  Per-trade outputs the mask
 * does not ask for are not written.  Blocks until the results are in the
 * (host) buffers.
 */
int adr_price(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades,
              uint32_t req_mask,
              double* pv, double* delta, double* gamma, double* agg);

/*
 * Same, with device-resident outputs and no host synchronisation: the kernels
 * are enqueued on `stream` (a hipStream_t; NULL = the ctx's own stream) and the
 * call returns immediately.  Output pointers are device memory owned by the
 * caller.  This is the entry the throughput benchmark times.  The call does no device
 * allocation and no synchronisation, so a sequence of them (a scenario ladder, the pieces
 * of a cross-currency book) can be captured on `stream` into a HIP graph and replayed.
 * (The first call for a (curve class, request) on a batch builds the batch's host-side
 * launch plan; later calls replay it.  Concurrent calls each hold the plan they walk.)
 * Stream rules: (1) a call with agg_dev != NULL stages its per-block partial sums in scratch
 * owned by the ctx, so all aggregate-producing calls of one ctx must be ordered on ONE
 * stream (or separated by a synchronisation); use one ctx per stream for concurrent aggregates.
 * (2) A batch that holds payment-lag or weighted coupons owns a per-wave scratch used by GAMMA requests:
 * calls with GAMMA on the SAME adr_trades must be stream-ordered.  Everything else - different batches on
 * different streams, calls without agg_dev - may run concurrently on one ctx.
 * (3) A batch with active schedule groups (adr_trades_set_schedule_groups) prices through per-batch basis buffers, but
 * only in calls with GAMMA, a per-trade gamma pointer and agg_dev != NULL - calls rule (1) already serialises; every other
 * call takes the direct route and stays free to run concurrently.
 */
int adr_price_dev(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades,
                  uint32_t req_mask,
                  double* pv_dev, double* delta_dev, double* gamma_dev, double* agg_dev,
                  void* stream);

/*
 * The foreign leg of a book of cross-currency swaps on TWO curves, one launch: Engine._compute_xccy's second leg call
 * (cavour/market/position/engine.py:1640-1733 - _float_leg_jax with the foreign OIS curve as index curve and the XCCY curve
 * as discount curve) with its two first-order ladders.  `legs` is an ordinary batch (adr_trades_upload): per swap the
 * foreign float coupons with flt_tp = payment times in the XCCY curve's day count, flt_ts / flt_te / flt_alpha in the
 * leg's own, the notional exchanges as fixed flows (times in the XCCY curve's day count), notional, spread and signs in
 * FOREIGN currency (the caller converts the results with 1 / spot, as the reference does at :1713, :1733).  A coupon is
 * N ((D_f(ts) / D_f(te) - 1) + spread alpha) D_x(tp): pv [n]; delta_foreign [n * P_f] = d pv / d (foreign par rates) with the
 * XCCY curve held fixed (:1702-1712); delta_basis [n * P_x] = d pv / d (basis spreads); per bp.  agg_foreign / agg_basis: the
 * book sums in adr_price's layout ([pv, delta[P], zeros]; the PV total sits in agg_foreign[0], agg_basis[0] is +0.0; without
 * ADR_REQ_DELTA in req_mask words 1 .. P of both are +0.0, as adr_price returns a block that is not asked for).  VALUE / DELTA only
 * (ADR_ERR_UNSUPPORTED with GAMMA: use three batches - adr_trades_upload_weighted - and adr_price); both curves up to 32
 * pillars, both on LINEAR_FWD_RATES or both on a log-linear scheme; every leg at most 390 coupons with some accrual end != payment time.
 * The _dev form enqueues on `stream` and neither allocates nor synchronises.
 */
int adr_price_xccy_foreign(adr_ctx* ctx, const adr_curve* foreign_curve, const adr_curve* xccy_curve, const adr_trades* legs,
                           uint32_t req_mask, double* pv, double* delta_foreign, double* delta_basis, double* agg_foreign,
                           double* agg_basis);
int adr_price_xccy_foreign_dev(adr_ctx* ctx, const adr_curve* foreign_curve, const adr_curve* xccy_curve, const adr_trades* legs,
                               uint32_t req_mask, double* pv_dev, double* delta_foreign_dev, double* delta_basis_dev,
                               double* agg_foreign_dev, double* agg_basis_dev, void* stream);

/*
 * Host-side half of adr_price_dev's routing, exposed so that it can be checked without a GPU (like adr_curve_layout_host):
 * the curve class, trade layout and launch plan the upload and adr_price_dev compute (route.hpp), for a curve (arguments as adr_curve_upload_ex) and a batch (the arrays of adr_trades_upload_weighted the
 * classification reads) under a request - req_mask, per_trade != 0: some per-trade output is wanted, aggregate != 0: agg is
 * wanted - on a device of n_cu compute units.  launches [max_launches][4] receives {kernel family, trade set, items,
 * blocks} per launch (enums of adrates_amd/csrc/route.hpp), cover [n] how many launches price each trade (the tile
 * launches of one pass count once): the library's contract is cover[i] == 1 for every trade.  Returns the number of
 * launches (possibly > max_launches) or a negative status.
 */
int adr_route_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac, const double* hess,
                   uint32_t curve_flags, int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* flt_tp,
                   const double* flt_te, const double* flt_alpha, const double* flt_weight, uint32_t req_mask, int per_trade,
                   int aggregate, int n_cu, int32_t* cover, int32_t* launches, int max_launches);

/*
 * Discount factors at n query times off an uploaded curve: InterpolatorAd.simple_interpolate evaluated on the GPU
 * (cavour/market/curves/interpolator_ad.py:186-249; same snap / + 1e-12 / duplicate-knot semantics as the pricing
 * kernels, all three schemes).  Replaces the reference's df lookups inside the cross-currency leg function
 * (cavour/market/position/engine.py:1640-1712: D_x(tp_j), D_f(ts_j), D_f(te_j)).  adr_curve_df takes and fills host
 * arrays and blocks; adr_curve_df_dev takes device arrays and enqueues on `stream` (NULL = the ctx's own).
 */
int adr_curve_df(adr_ctx* ctx, const adr_curve* curve, int64_t n, const double* t, double* df);
int adr_curve_df_dev(adr_ctx* ctx, const adr_curve* curve, int64_t n, const double* t_dev, double* df_dev, void* stream);

/*
 * Spread and yield measures of fixed-rate bonds, one root-find pair per bond (cavour/trades/credit/bond.py:262-783, the
 * host methods of adrates_amd/trades/credit/bond.py).  Discount factors come from the curve's OWN nodes (node_t ascending,
 * node_df; interpolator.py::_point), not from an uploaded engine curve.
 *
 * Flows (CSR over bonds, flow_off [n + 1]; only flows paid after settlement): flow_T the curve time of the payment date
 * (ACT/ACT ISDA from the curve's value date, as DiscountCurve.df), flow_tau = (payment - settlement) days / 365.25, the
 * coupon and the principal amount (a principal <= 0 is not paid, as in Bond.value).  Per bond: bond_Ts the curve time of
 * settlement, bond_tauM = (unadjusted maturity - settlement) / 365.25 (<= 0: matured; the yield measures price the FULL
 * face there, ignoring amortization), the face, the accrued interest per 100 face, and the quote: a clean price per 100
 * (quote_is_z = 0; z is solved) or a z-spread (quote_is_z = 1).
 *
 * out [ADR_BOND_OUTPUTS][n], row k = ADR_BOND_* below.  status [n]: 0 = the bracket ([-0.1, 0.5] for z, [-0.5, 0.5] for
 * the yield) held a sign change and a bracketed safeguarded Newton solved it; 1 = no sign change and the unbracketed Newton
 * fallback (from 0.01 / 0.05) converged; 2 = no root: the outputs depending on it are NaN.  Duration is Macaulay; dv01 is
 * the central 1bp difference in z, which is also cs01.  Results are bit-identical from run to run and do not depend on
 * the launch shape; adr_bond_measures_host runs the same per-bond code and reduction order on the CPU (no GPU needed).
 */
#define ADR_BOND_OUTPUTS 7
#define ADR_BOND_Z 0
#define ADR_BOND_DIRTY 1
#define ADR_BOND_CLEAN 2
#define ADR_BOND_YTM 3
#define ADR_BOND_DURATION 4
#define ADR_BOND_CONVEXITY 5
#define ADR_BOND_DV01 6
#define ADR_BOND_MAX_NODES 1024
int adr_bond_measures(adr_ctx* ctx, int interp_method, int n_nodes, const double* node_t, const double* node_df, int64_t n,
                      const int64_t* flow_off, const double* flow_T, const double* flow_tau, const double* flow_cpn,
                      const double* flow_prin, const double* bond_Ts, const double* bond_tauM, const double* bond_face,
                      const double* bond_acc100, const double* bond_quote, int quote_is_z, double* out, int32_t* status);
/* The same with every array in device memory, enqueued on `stream` (NULL: the ctx's stream); only the scalars are checked. */
int adr_bond_measures_dev(adr_ctx* ctx, int interp_method, int n_nodes, const double* node_t, const double* node_df, int64_t n,
                          const int64_t* flow_off, const double* flow_T, const double* flow_tau, const double* flow_cpn,
                          const double* flow_prin, const double* bond_Ts, const double* bond_tauM, const double* bond_face,
                          const double* bond_acc100, const double* bond_quote, int quote_is_z, double* out, int32_t* status,
                          void* stream);
int adr_bond_measures_host(int interp_method, int n_nodes, const double* node_t, const double* node_df, int64_t n,
                           const int64_t* flow_off, const double* flow_T, const double* flow_tau, const double* flow_cpn,
                           const double* flow_prin, const double* bond_Ts, const double* bond_tauM, const double* bond_face,
                           const double* bond_acc100, const double* bond_quote, int quote_is_z, double* out, int32_t* status);

/*
 * Discount margins, prices, modified durations and dv01s of floating-rate notes, one root find per FRN
 * (cavour/trades/credit/frn.py:235-614, the host methods of adrates_amd/trades/credit/frn.py).  Discount factors come
 * from two curves' OWN node sets (node_t ascending, node_df; interpolator.py::_point), each with its own scheme: the
 * discount curve and the index curve the forwards are projected on (they may be the same curve).
 *
 * Coupons (CSR over FRNs, cpn_off [n + 1] from 0 to m; only coupons paid after settlement): cpn [ADR_FRN_FLOW_FIELDS][m],
 * row k = ADR_FRN_CPN_* below - the discount-curve time of the payment; the index-curve times of the accrual start and
 * end; the index curve's year fraction of the period (the forward's divisor) and the FRN's (the coupon's); the DM time
 * yf_frn(settlement, payment); and 1 where the first-fixing rate replaces the forward (0 otherwise).  Curve times are year
 * fractions in the FRN's day count from each curve's value date, as DiscountCurve.df(dt, frn._dc_type) reads them.
 * Per FRN: frn [ADR_FRN_FIELDS][n], row k = ADR_FRN_* below - the discount-curve time of settlement, the discount-curve
 * time and the DM time of the principal at the adjusted maturity (time NaN: matured, no principal), the face, the margin,
 * the cap and the floor (+inf / -inf: none), the first-fixing rate, the accrued interest per 100 face, the quote - a clean
 * price per 100 (quote_is_dm = 0; the DM is solved) or a DM (quote_is_dm = 1) - and the fallback solver's start.
 *
 * Per FRN each coupon is projected once (forward or fixing, + margin, cap, floor, x FRN year fraction x face) and kept as
 * amount * D(pay) / D(settlement); the price at DM x discounts each flow by a further exp(-x tau).  out [ADR_FRN_OUTPUTS][n],
 * row k = ADR_FRN_* outputs below: the DM, dirty and clean prices per 100, the PV in currency, the modified duration (the
 * central +-1bp DM difference of dirty prices over the price) and dv01 = |PV(DM + 1bp) - PV(DM)|.  status [n]: 0 = the
 * bracket [-0.10, 0.20] held a sign change and a bracketed safeguarded Newton solved it (also when the DM is given);
 * 1 = no sign change and the unbracketed Newton fallback from the start converged; 2 = no root: every output is NaN;
 * 3 = not priceable, a coupon's forward needs the index curve before its first node (FRN.value raises): every output
 * is NaN.  Results are bit-identical from run to run and do not depend on the launch shape; adr_frn_measures_host runs
 * the same per-FRN code and reduction order on the CPU (no GPU needed).
 */
#define ADR_FRN_FLOW_FIELDS 7
#define ADR_FRN_CPN_T 0
#define ADR_FRN_CPN_TS 1
#define ADR_FRN_CPN_TE 2
#define ADR_FRN_CPN_IALPHA 3
#define ADR_FRN_CPN_ALPHA 4
#define ADR_FRN_CPN_TAU 5
#define ADR_FRN_CPN_FIX 6
#define ADR_FRN_FIELDS 11
#define ADR_FRN_TS 0
#define ADR_FRN_TM 1
#define ADR_FRN_TAUM 2
#define ADR_FRN_FACE 3
#define ADR_FRN_MARGIN 4
#define ADR_FRN_CAP 5
#define ADR_FRN_FLOOR 6
#define ADR_FRN_FFR 7
#define ADR_FRN_ACC100 8
#define ADR_FRN_QUOTE 9
#define ADR_FRN_GUESS 10
#define ADR_FRN_OUTPUTS 6
#define ADR_FRN_DM 0
#define ADR_FRN_DIRTY 1
#define ADR_FRN_CLEAN 2
#define ADR_FRN_PV 3
#define ADR_FRN_MOD_DURATION 4
#define ADR_FRN_DV01 5
#define ADR_FRN_MAX_NODES 1024
int adr_frn_measures(adr_ctx* ctx, int disc_method, int disc_n, const double* disc_t, const double* disc_df,
                     int index_method, int index_n, const double* index_t, const double* index_df, int64_t n, int64_t m,
                     const int64_t* cpn_off, const double* cpn, const double* frn, int quote_is_dm, double* out,
                     int32_t* status);
/* The same with every array in device memory, enqueued on `stream` (NULL: the ctx's stream); only the scalars are checked. */
int adr_frn_measures_dev(adr_ctx* ctx, int disc_method, int disc_n, const double* disc_t, const double* disc_df,
                         int index_method, int index_n, const double* index_t, const double* index_df, int64_t n, int64_t m,
                         const int64_t* cpn_off, const double* cpn, const double* frn, int quote_is_dm, double* out,
                         int32_t* status, void* stream);
int adr_frn_measures_host(int disc_method, int disc_n, const double* disc_t, const double* disc_df, int index_method,
                          int index_n, const double* index_t, const double* index_df, int64_t n, int64_t m,
                          const int64_t* cpn_off, const double* cpn, const double* frn, int quote_is_dm, double* out,
                          int32_t* status);

/*
 * Year-on-year inflation swaps: the inflation leg's projected amounts, PV and inflation-curve delta / gamma
 * (cavour/market/position/engine.py:986-1353, `_compute_yoy_iis`, with the discount curve held fixed).
 *
 * The discount curve is the engine's knot grid: `disc_method` (1, 2 or 4), K (2 .. ADR_YOY_MAX_KNOTS) knot times[K]
 * (non-decreasing, t = 0 first; repeats allowed) and dfs[K].  The inflation curve is given by its P (1 ..
 * ADR_YOY_MAX_PILLARS) pillars: `infl_method` (ADR_INTERP_LINEAR_ZERO_RATES or ADR_INTERP_FLAT_FWD_RATES; anything else
 * is ADR_ERR_UNSUPPORTED), times T[P] (0 < T_1 < ... ) and breakeven rates b[P]; the kernel forms the nodes (0, 1),
 * (T_k, (1 + b_k)^T_k).  Both curves are read as InterpolatorAd.simple_interpolate reads them.
 *
 * Coupons in CSR form: swap i owns coupons cpn_off[i] .. cpn_off[i+1]-1 of the field-major cpn[ADR_YOY_FIELDS][m]:
 * payment time tp, YoY start ts and end te (years from the value date), scale = leg sign * notional * accrual fraction
 * and spread.  Per coupon, with 1 + y = I(te) / I(ts):
 *     amount = scale * (y + spread),   PV += amount * D(tp) / D(0)  when tp > 0.
 * Outputs (NULL where not wanted): amount[m] (always written when given), and by req_mask - ADR_REQ_VALUE / _DELTA /
 * _GAMMA choose the measures, ADR_YOY_PER_SWAP writes per-swap rows pv[n], delta[n][P] (per bp) and gamma[n][P][P]
 * (per bp^2, dense, row-major), ADR_YOY_AGG writes agg[1 + P + P*P] = [pv, delta[P], gamma[P*P]] of the whole book.
 * agg is a fixed-order sum of the per-swap rows: swaps in chunks of ADR_YOY_CHUNK summed in order, then chunk j added
 * to lane j % 64 in order, then lanes 0-31 += 32-63, 0-15 += 16-31, ..., 0 += 1.  Results are bit-identical from run to run and do
 * not depend on the launch shape or the batch; adr_yoy_risk_host runs the same per-swap code and order on the CPU.
 * With ADR_YOY_AGG every entry of agg is written: the slots of a measure that req_mask does not name hold 0.0, and
 * n = 0 gives an all-zero agg.  An output that req_mask does not ask for is never written, whether or not its pointer
 * is given; amount is written without ADR_YOY_PER_SWAP and ADR_YOY_AGG too.  adr_yoy_risk_dev cannot refuse offsets it
 * has not read: a swap whose cpn_off pair is negative, decreasing or ends beyond m reads no coupon and gets a NaN PV
 * (zero delta and gamma rows), which carries into agg[0].
 */
#define ADR_YOY_FIELDS 5
#define ADR_YOY_TP 0
#define ADR_YOY_TS 1
#define ADR_YOY_TE 2
#define ADR_YOY_SCALE 3
#define ADR_YOY_SPREAD 4
#define ADR_YOY_MAX_KNOTS 4096
#define ADR_YOY_MAX_PILLARS 64
#define ADR_YOY_CHUNK 16
#define ADR_YOY_PER_SWAP 8u
#define ADR_YOY_AGG 16u
int adr_yoy_risk(adr_ctx* ctx, int disc_method, int K, const double* times, const double* dfs, int infl_method, int P,
                 const double* T, const double* b, int64_t n, int64_t m, const int64_t* cpn_off, const double* cpn,
                 uint32_t req_mask, double* amount, double* pv, double* delta, double* gamma, double* agg);
/* Doubles of scratch adr_yoy_risk_dev needs for ADR_YOY_AGG: ceil(n / ADR_YOY_CHUNK) * (1 + P + P*P). */
int64_t adr_yoy_risk_work(int64_t n, int P);
/* The same with every array in device memory (work: adr_yoy_risk_work doubles, or NULL without ADR_YOY_AGG),
 * enqueued on `stream` (NULL: the ctx's stream); no allocation, no synchronisation; only the scalars are checked. */
int adr_yoy_risk_dev(adr_ctx* ctx, int disc_method, int K, const double* times, const double* dfs, int infl_method, int P,
                     const double* T, const double* b, int64_t n, int64_t m, const int64_t* cpn_off, const double* cpn,
                     uint32_t req_mask, double* amount, double* pv, double* delta, double* gamma, double* agg,
                     double* work, void* stream);
int adr_yoy_risk_host(int disc_method, int K, const double* times, const double* dfs, int infl_method, int P,
                      const double* T, const double* b, int64_t n, int64_t m, const int64_t* cpn_off, const double* cpn,
                      uint32_t req_mask, double* amount, double* pv, double* delta, double* gamma, double* agg);

/*
 * Scenario revaluation: the PV of every trade of an uploaded batch under S discount curves that share one knot grid -
 * the P&L vectors behind historical-simulation VaR, expected shortfall and stress tests.  The reference revalues one
 * Model.scenario at a time (cavour/models/models.py:507-557: a new model, bootstrap and trace per shock).
 *
 * Curves: interp_method (1, 2 or 4), K (2 .. ADR_SCENARIO_MAX_KNOTS) knot times[K] (non-decreasing, repeats allowed; the
 * first knot is the value-time point t = 0 with discount factor 1, as for adr_curve_upload: the PV is not divided by
 * D(0)) and dfs[S][K], one row of positive discount factors per scenario (S >= 1).  No rates and no Jacobians: the rows
 * may come from the device curve builder (adr_curve_set_arrays) or from anywhere else.
 *
 * pv[i][s] - TRADE-major, [n][S], or NULL - is what adr_price(VALUE) returns for trade i on the curve (times, dfs[s]):
 *     fix_sign * sum_j pay_j D_s(tp_j) [tp_j > 0]
 *   + flt_sign * N * sum_j w_j ((D_s(ts_j) / D_s(te_j) - 1) [alpha_j > 0] + spread alpha_j) D_s(tp_j) [tp_j >= 0],
 * D_s(t) = InterpolatorAd.simple_interpolate on row s; every batch adr_price accepts (payment lag, flt_weight, legs of
 * any length).  book_pv[s] = sum_i pv[i][s] in a fixed order: the trades in chunks of ADR_SCENARIO_CHUNK summed in
 * trade order from 0.0, then chunk j added to slot j % 64 in order, then slots 0-31 += 32-63, 0-15 += 16-31, ..., 0 += 1.
 * A scenario's results do not depend on S, on the other scenarios or on the launch shape, and are bit-identical from
 * run to run; adr_scenario_pv_host runs the same per-trade arithmetic in the same order on CPU threads (no GPU needed;
 * n_threads <= 0: as many as the machine suggests, at most 16) and differs from the device by exp / log only.
 *
 * adr_scenario_pv: host arrays in and out, blocks.  adr_scenario_pv_dev: device arrays, enqueued on `stream` (NULL: the
 * ctx's own), no allocation and no synchronisation (capturable into a HIP graph: two kernels in one chain); work_dev
 * holds adr_scenario_pv_work(n, S) doubles; only the scalars are checked.  adr_scenario_pv_set: the curves of a set built
 * by adr_curve_set_build, read where they are; host outputs, blocks.  adr_curve_set_arrays: that set's scheme, K, S and
 * the device pointers of its knot times [K] and discount factors [S][K] (any output may be NULL) for adr_scenario_pv_dev.
 */
#define ADR_SCENARIO_MAX_KNOTS 4096
#define ADR_SCENARIO_CHUNK 64
int adr_scenario_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S, const double* dfs,
                    const adr_trades* trades, double* pv, double* book_pv);
/* Doubles of scratch adr_scenario_pv_dev needs: ceil(n / ADR_SCENARIO_CHUNK) * S. */
int64_t adr_scenario_pv_work(int64_t n, int S);
int adr_scenario_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S, const double* dfs_dev,
                        const adr_trades* trades, double* pv_dev, double* book_pv_dev, double* work_dev, void* stream);
int adr_scenario_pv_set(adr_ctx* ctx, const adr_curve_set* set, const adr_trades* trades, double* pv, double* book_pv);
int adr_curve_set_arrays(const adr_curve_set* set, int* interp_method, int* K, int* S, const double** times_dev,
                         const double** dfs_dev);
/* The trades as the arrays of adr_trades_upload_weighted (flt_weight may be NULL). */
int adr_scenario_pv_host(int interp_method, int K, const double* times, int S, const double* dfs, int64_t n,
                         const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                         const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                         const double* flt_weight, const double* notional, const double* spread, const double* fix_sign,
                         const double* flt_sign, double* pv, double* book_pv, int n_threads);

/*
 * Inflation scenario revaluation: the PV of every YoY inflation swap of a book under S scenarios, each a PAIR of a
 * discount curve row and a breakeven row - VaR, expected shortfall and stress P&L under joint rates-and-breakeven
 * shocks in one launch, instead of one adr_yoy_risk, one host pass and one adr_price per scenario.
 *
 *     pv[i][s] =  sum_f fix_pay_f D_s(tp_f)                                          [tp_f > 0]
 *               + sum_j scale_j (I_s(te_j) / I_s(ts_j) - 1 + spread_j) D_s(tp_j)     [tp_j > 0]     (both masks strict)
 *     book_pv[s] = sum_i pv[i][s]
 *
 * D_s(t): InterpolatorAd.simple_interpolate on (times[K], dfs[s][K]), disc_method 1, 2 or 4, as adr_scenario_pv reads it
 * (the first knot is t = 0 with discount factor 1; no division by D(0); K = 2 .. ADR_SCENARIO_MAX_KNOTS).  I_s(t): the
 * same rule on the nodes (0, 1), (T_k, (1 + b[s][k])^T_k), infl_method ADR_INTERP_LINEAR_ZERO_RATES or
 * ADR_INTERP_FLAT_FWD_RATES (anything else is ADR_ERR_UNSUPPORTED), P = 1 .. ADR_YOY_MAX_PILLARS, formed as adr_yoy_risk
 * forms them: for one scenario the projected amounts are adr_yoy_risk's up to the rounding of one exponent.
 *
 * Broadcasting: S_disc and S_infl are each 1 or S.  One shared row means "this curve is not shocked" and is read with
 * stride 0: discount-only, inflation-only and joint scenarios from one entry.
 *
 * The book, n >= 1 swaps: the fixed legs in CSR form fix_off[n+1], fix_tp[n_fix], fix_pay[n_fix] (signs folded in, the
 * principal on the last flow) and the YoY coupons as adr_yoy_risk takes them, cpn_off[n+1] and the field-major
 * cpn[ADR_YOY_FIELDS][m].  Either leg may be empty, for a swap or for the whole book (offsets of 0; the value arrays
 * may then be NULL).  Within a swap, index c = 0, 1, ... adds coupon c to the YoY sum and fixed flow c to the fixed
 * sum, each in order from 0.0; pv = fixed sum + YoY sum.
 *
 * Outputs: book_pv[S] always; pv[n][S] (swap-major, the layout of adr_scenario_pv) when given.  book_pv follows
 * adr_scenario_pv's rule: the swaps in chunks of ADR_SCENARIO_CHUNK summed in order from 0.0, chunk j added to slot
 * j % 64 in order, then slots 0-31 += 32-63, ..., 0 += 1; no atomics.  A scenario's results do not depend on S, on the
 * other scenarios, on broadcasting or on the launch shape, and are bit-identical from run to run.
 *
 * adr_yoy_scenario_pv: host arrays in and out, blocks; refuses what it can read (offsets that do not run from 0 to
 * the count or decrease, non-finite times or amounts, 1 + b <= 0, non-positive discount factors, T not increasing from
 * > 0).  adr_yoy_scenario_pv_dev: device arrays, enqueued on `stream` (NULL: the ctx's own), no allocation and no
 * synchronisation (two kernels in one chain); work_dev holds adr_yoy_scenario_pv_work(n, S) doubles; only the scalars
 * are checked: a swap whose offset pair is negative, decreasing or ends beyond the count reads no flow and gets a NaN
 * PV, which carries into book_pv.  adr_yoy_scenario_pv_host: the same per-date and per-coupon code in the same order on
 * CPU threads (no GPU; n_threads <= 0: as many as the machine suggests, at most 16); it differs from the device by
 * exp / log only.
 */
int adr_yoy_scenario_pv(adr_ctx* ctx, int disc_method, int K, const double* times, int S_disc, const double* dfs,
                        int infl_method, int P, const double* T, int S_infl, const double* b, int S, int64_t n, int64_t n_fix,
                        const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m, const int64_t* cpn_off,
                        const double* cpn, double* pv, double* book_pv);
/* Doubles of scratch adr_yoy_scenario_pv_dev needs: ceil(n / ADR_SCENARIO_CHUNK) * S. */
int64_t adr_yoy_scenario_pv_work(int64_t n, int S);
int adr_yoy_scenario_pv_dev(adr_ctx* ctx, int disc_method, int K, const double* times_dev, int S_disc, const double* dfs_dev,
                            int infl_method, int P, const double* T_dev, int S_infl, const double* b_dev, int S, int64_t n,
                            int64_t n_fix, const int64_t* fix_off_dev, const double* fix_tp_dev, const double* fix_pay_dev,
                            int64_t m, const int64_t* cpn_off_dev, const double* cpn_dev, double* pv_dev, double* book_pv_dev,
                            double* work_dev, void* stream);
int adr_yoy_scenario_pv_host(int disc_method, int K, const double* times, int S_disc, const double* dfs, int infl_method,
                             int P, const double* T, int S_infl, const double* b, int S, int64_t n, int64_t n_fix,
                             const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                             const int64_t* cpn_off, const double* cpn, double* pv, double* book_pv, int n_threads);

/*
 * Cross-currency scenario revaluation: the PV of the FOREIGN leg of every cross-currency swap of an uploaded batch under
 * S scenarios, each a PAIR of a foreign OIS row (the forwards) and an XCCY row (the discount factors) - the launch that
 * replaces, per scenario, two curve uploads and one adr_price_xccy_foreign.  The domestic legs are an ordinary batch on one
 * curve: adr_scenario_pv.
 *
 *     pv[i][s] = fix_sign_i * sum_j pay_j Dx_s(tp_j)                                                          [tp_j > 0]
 *              + flt_sign_i * N_i * sum_j w_j ((Df_s(ts_j) / Df_s(te_j) - 1) [alpha_j > 0] + spread_i alpha_j) Dx_s(tp_j)
 *                                                                                                             [tp_j >= 0]
 *     book_pv[s] = sum_i pv[i][s]
 *
 * Df_s(t): InterpolatorAd.simple_interpolate on (times_f[K_f], dfs_f[s][K_f]) with for_method; Dx_s(t): the same rule on
 * (times_x[K_x], dfs_x[s][K_x]) with x_method; each grid as adr_scenario_pv reads it (the first knot is t = 0 with discount
 * factor 1; no division by D(0); 2 .. ADR_SCENARIO_MAX_KNOTS knots, non-decreasing, repeats allowed).  `legs` is the batch
 * adr_price_xccy_foreign takes (adr_trades_upload_weighted): flt_ts / flt_te / flt_alpha in the foreign leg's day count,
 * flt_tp and the notional exchanges (fixed flows) in the XCCY curve's, amounts in FOREIGN currency; the caller converts
 * with 1 / spot.  The masks, flt_weight, the per-trade sum order (coupon c and fixed flow c at index c, each sum from
 * 0.0) and the final fix_sign * fixed + (flt_sign * N) * float + 0.0 are adr_scenario_pv's: with one table and one scheme
 * passed as both curves, adr_xccy_scenario_pv_host returns adr_scenario_pv_host's bits.
 *
 * Scheme pairs: both curves on ADR_INTERP_LINEAR_FWD_RATES, or each on ADR_INTERP_FLAT_FWD_RATES or
 * ADR_INTERP_LINEAR_ZERO_RATES (four pairs).  LINEAR_FWD_RATES beside a log-linear scheme is ADR_ERR_UNSUPPORTED, as in
 * adr_price_xccy_foreign.
 *
 * Broadcasting: S_f and S_x are each 1 or S.  One shared row means "this curve is not shocked" and is read with stride
 * 0: foreign-only, basis-only and joint scenarios from one entry.
 *
 * Outputs: book_pv[S] always; pv[n][S] (trade-major, the layout of adr_scenario_pv) when given.  book_pv follows
 * adr_scenario_pv's rule: the trades in chunks of ADR_SCENARIO_CHUNK summed in order from 0.0, chunk j added to slot
 * j % 64 in order, then slots 0-31 += 32-63, ..., 0 += 1; no atomics.  A scenario's results do not depend on S, on the
 * other scenarios, on broadcasting, on which tables sit in LDS or on the launch shape, and are bit-identical from run to
 * run.
 *
 * adr_xccy_scenario_pv: host curves in, host outputs, blocks; refuses knot times that are not finite and non-decreasing
 * and discount factors that are not positive and finite.  adr_xccy_scenario_pv_dev: device arrays, enqueued on `stream`
 * (NULL: the ctx's own), no allocation and no synchronisation (two kernels in one chain); work_dev holds
 * adr_xccy_scenario_pv_work(n, S) doubles; only the scalars are checked.  adr_xccy_scenario_pv_host: the legs as the arrays
 * of adr_trades_upload_weighted (flt_weight may be NULL), checked as adr_scenario_pv_host checks them; the same per-date
 * and per-coupon code in the same order on CPU threads (no GPU; n_threads <= 0: as many as the machine suggests, at most
 * 16); it differs from the device by exp / log only.
 *
 * Sub-books: the _subbook entries take in addition B >= 1, sub_off[B + 1] (the _dev form: the uploaded plan of
 * adr_scenario_subbook_plan and adr_scenario_subbook_work(n, B, S) doubles of scratch; three kernels) and return
 * sub_pv[B][S] under the contract of adr_scenario_subbook_pv, word for word: sub_pv[b][s] has exactly the bits of
 * adr_xccy_scenario_pv's book_pv[s] on a batch holding sub-book b's trades alone; an empty sub-book gives +0.0; pv[n][S],
 * when given, has the parent's bits.
 */
int adr_xccy_scenario_pv(adr_ctx* ctx, int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f, int x_method,
                         int K_x, const double* times_x, int S_x, const double* dfs_x, int S, const adr_trades* legs, double* pv,
                         double* book_pv);
/* Doubles of scratch adr_xccy_scenario_pv_dev needs: ceil(n / ADR_SCENARIO_CHUNK) * S. */
int64_t adr_xccy_scenario_pv_work(int64_t n, int S);
int adr_xccy_scenario_pv_dev(adr_ctx* ctx, int for_method, int K_f, const double* times_f_dev, int S_f, const double* dfs_f_dev,
                             int x_method, int K_x, const double* times_x_dev, int S_x, const double* dfs_x_dev, int S,
                             const adr_trades* legs, double* pv_dev, double* book_pv_dev, double* work_dev, void* stream);
int adr_xccy_scenario_pv_host(int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f, int x_method, int K_x,
                              const double* times_x, int S_x, const double* dfs_x, int S, int64_t n, const int64_t* fix_off,
                              const int64_t* flt_off, const double* fix_tp, const double* fix_pay, const double* flt_tp,
                              const double* flt_ts, const double* flt_te, const double* flt_alpha, const double* flt_weight,
                              const double* notional, const double* spread, const double* fix_sign, const double* flt_sign,
                              double* pv, double* book_pv, int n_threads);
int adr_xccy_scenario_subbook_pv(adr_ctx* ctx, int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f,
                                 int x_method, int K_x, const double* times_x, int S_x, const double* dfs_x, int S,
                                 const adr_trades* legs, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv);
int adr_xccy_scenario_subbook_pv_dev(adr_ctx* ctx, int for_method, int K_f, const double* times_f_dev, int S_f,
                                     const double* dfs_f_dev, int x_method, int K_x, const double* times_x_dev, int S_x,
                                     const double* dfs_x_dev, int S, const adr_trades* legs, int64_t B, const int64_t* plan_dev,
                                     double* pv_dev, double* sub_pv_dev, double* work_dev, void* stream);
int adr_xccy_scenario_subbook_pv_host(int for_method, int K_f, const double* times_f, int S_f, const double* dfs_f, int x_method,
                                      int K_x, const double* times_x, int S_x, const double* dfs_x, int S, int64_t n,
                                      const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                                      const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                                      const double* flt_weight, const double* notional, const double* spread,
                                      const double* fix_sign, const double* flt_sign, int64_t B, const int64_t* sub_off,
                                      double* pv, double* sub_pv, int n_threads);

/*
 * Credit scenario revaluation: the PV of every trade of an uploaded batch under S scenarios, each a PAIR of a discount
 * curve row and a row of spread shocks per credit bucket - bonds at their z-spreads and FRNs at their discount margins
 * under rate-only, spread-only and joint shocks in one launch, instead of one rescaled upload and one adr_price per
 * scenario.
 *
 *     x[i][s]  = z[i] + (bucket[i] >= 0 ? dz[s][bucket[i]] : 0)
 *     pv[i][s] = fix_sign_i * sum_f fix_pay_f D_s(tp_f) exp(-x fix_tau_f)                                  [tp_f > 0]
 *              + flt_sign_i * N_i * sum_j w_j ((D_s(ts_j) / D_s(te_j) - 1) [alpha_j > 0] + spread_i alpha_j)
 *                                         D_s(tp_j) exp(-x flt_tau_j)                                      [tp_j >= 0]
 *     book_pv[s] = sum_i pv[i][s]
 *
 * D_s(t), the masks and the alpha <= 0 rule are adr_scenario_pv's (interp_method 1, 2 or 4; K = 2 ..
 * ADR_SCENARIO_MAX_KNOTS; the first knot is t = 0; no division by D(0)).  The forward D(ts) / D(te) carries no spread;
 * only the payment's discount factor does.  Under the log-linear schemes -x tau joins the exponent of D(tp), so a flow
 * costs one exp.  A trade with z = 0 and bucket = -1 is priced by adr_scenario_pv's own arithmetic.
 *
 * New inputs: per trade z[n] (finite) and bucket[n] (-1: no shock, or 0 .. G - 1); per fixed flow fix_tau[n_fix] and per
 * float coupon flt_tau[n_flt], the spread times, in the order of the batch's flow arrays (n_fix and n_flt are the
 * batch's flow counts); per scenario dz[S_spr][G], G = 0 .. ADR_CREDIT_MAX_BUCKETS (dz may be NULL when G = 0).
 *
 * Broadcasting: S_disc and S_spr are each 1 or S.  One shared row means "not shocked" and is read with stride 0.
 *
 * Outputs: book_pv[S] always; pv[n][S] (trade-major) when given.  book_pv follows adr_scenario_pv's rule: the trades in
 * chunks of ADR_SCENARIO_CHUNK summed in order from 0.0, chunk j added to slot j % 64 in order, then slots 0-31 += 32-63,
 * ..., 0 += 1; no atomics.  A scenario's results do not depend on S, on the other scenarios, on broadcasting or on the
 * launch shape, and are bit-identical from run to run.
 *
 * adr_credit_scenario_pv: host arrays in and out, blocks; refuses what it can read (non-finite z, dz or spread times,
 * a bucket outside -1 .. G - 1, non-positive discount factors, knot times that decrease, a broadcast count other than
 * 1 or S).  adr_credit_scenario_pv_set: the same with the curves of a set built by adr_curve_set_build, read where
 * adr_curve_set_arrays finds them (S and S_disc are the set's count).  adr_credit_scenario_pv_dev: device arrays,
 * enqueued on `stream` (NULL: the ctx's own), no allocation and no synchronisation (two kernels in one chain); work_dev
 * holds adr_credit_scenario_pv_work(n, S) doubles; only the scalars are checked: a trade whose flows do not lie inside
 * 0 .. n_fix / 0 .. n_flt, or whose bucket is outside -1 .. G - 1, reads no flow and gets a NaN PV, which carries into
 * book_pv.  adr_credit_scenario_pv_host: the trades as the arrays of adr_trades_upload_weighted, the same per-date and
 * per-coupon code in the same order on CPU threads (no GPU; n_threads <= 0: as many as the machine suggests, at most
 * 16); it differs from the device by exp / log only.
 */
#define ADR_CREDIT_MAX_BUCKETS 32
int adr_credit_scenario_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S_disc, const double* dfs, int G,
                           int S_spr, const double* dz, int S, const adr_trades* trades, const double* z, const int32_t* bucket,
                           int64_t n_fix, const double* fix_tau, int64_t n_flt, const double* flt_tau, double* pv,
                           double* book_pv);
int adr_credit_scenario_pv_set(adr_ctx* ctx, const adr_curve_set* set, int G, int S_spr, const double* dz,
                               const adr_trades* trades, const double* z, const int32_t* bucket, int64_t n_fix,
                               const double* fix_tau, int64_t n_flt, const double* flt_tau, double* pv, double* book_pv);
/* Doubles of scratch adr_credit_scenario_pv_dev needs: ceil(n / ADR_SCENARIO_CHUNK) * S. */
int64_t adr_credit_scenario_pv_work(int64_t n, int S);
int adr_credit_scenario_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S_disc, const double* dfs_dev,
                               int G, int S_spr, const double* dz_dev, int S, const adr_trades* trades, const double* z_dev,
                               const int32_t* bucket_dev, int64_t n_fix, const double* fix_tau_dev, int64_t n_flt,
                               const double* flt_tau_dev, double* pv_dev, double* book_pv_dev, double* work_dev, void* stream);
int adr_credit_scenario_pv_host(int interp_method, int K, const double* times, int S_disc, const double* dfs, int G, int S_spr,
                                const double* dz, int S, int64_t n, const int64_t* fix_off, const int64_t* flt_off,
                                const double* fix_tp, const double* fix_pay, const double* flt_tp, const double* flt_ts,
                                const double* flt_te, const double* flt_alpha, const double* flt_weight, const double* notional,
                                const double* spread, const double* fix_sign, const double* flt_sign, const double* z,
                                const int32_t* bucket, const double* fix_tau, const double* flt_tau, double* pv, double* book_pv,
                                int n_threads);

/*
 * Sub-books: the P&L vectors of B disjoint parts of a batch - desks, counterparties, margin accounts - from ONE launch
 * of the scenario kernels, and their tail measures on the device.  The entries mirror adr_scenario_pv* and
 * adr_credit_scenario_pv* and take everything their parents take, plus B >= 1 and sub_off[B + 1]: sub-book b holds the
 * trades sub_off[b] .. sub_off[b + 1] of the batch.  The offsets run from 0 to n and do not decrease; a sub-book may be
 * empty.  Outputs: sub_pv[B][S], row-major, always; pv[n][S] when given, with the parent's bits.
 *
 * sub_pv[b][s] has exactly the bits of the parent's book_pv[s] on a batch holding sub-book b's trades alone, in order:
 * chunk c of sub-book b is the trades sub_off[b] + 64 c .., summed in order from 0.0; the sub-book's chunk j is added to
 * slot j % 64 in order; then slots 0-31 += 32-63, ..., 0 += 1.  No atomics.  An empty sub-book's row is +0.0.  A row
 * does not depend on B, on the other sub-books, on S or on the launch shape, and is bit-identical from run to run.
 *
 * How the chunks reach the device: as a PLAN, B + 1 + 2 C int64 for C chunks, which the caller of a _dev entry fills on
 * the host with adr_scenario_subbook_plan and uploads (the blocking entries do both themselves).  plan[0 .. B] is the
 * prefix of the sub-books' chunk counts (plan[B] = C <= ceil(n / 64) + B), then come C pairs (first trade, one past the
 * last).  adr_scenario_subbook_plan(n, B, sub_off, plan) checks the offsets (ADR_ERR_INVALID naming the sub-book),
 * fills plan when it is not NULL and returns the plan's length in int64.  adr_scenario_subbook_work(n, B, S) is the
 * scratch of the _dev entries in doubles, (ceil(n / 64) + B) * S, for both families.
 *
 * The _dev entries take device arrays and the uploaded plan, enqueue on `stream` (NULL: the ctx's own) without
 * allocation or synchronisation (three kernels in one chain: pricing, and the sum for small and for large sub-books)
 * and check scalars only: a plan whose bounds leave 0 .. n is
 * cut to that range, one with more chunks than the scratch holds is cut there.  The host-array entries refuse offsets
 * that are not 0 .. n or that decrease.  The _host twins run the same code in the same order on CPU threads.
 * adr_scenario_subbook_var_es chains adr_scenario_tail_dev's kernel behind the launch: var[B] and es[B] come back, the
 * [B][S] rows never leave the device.
 */
int64_t adr_scenario_subbook_plan(int64_t n, int64_t B, const int64_t* sub_off, int64_t* plan);
int64_t adr_scenario_subbook_work(int64_t n, int64_t B, int S);
int adr_scenario_subbook_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S, const double* dfs,
                            const adr_trades* trades, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv);
int adr_scenario_subbook_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S, const double* dfs_dev,
                                const adr_trades* trades, int64_t B, const int64_t* plan_dev, double* pv_dev, double* sub_pv_dev,
                                double* work_dev, void* stream);
int adr_scenario_subbook_pv_set(adr_ctx* ctx, const adr_curve_set* set, const adr_trades* trades, int64_t B, const int64_t* sub_off,
                                double* pv, double* sub_pv);
int adr_scenario_subbook_pv_host(int interp_method, int K, const double* times, int S, const double* dfs, int64_t n,
                                 const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp, const double* fix_pay,
                                 const double* flt_tp, const double* flt_ts, const double* flt_te, const double* flt_alpha,
                                 const double* flt_weight, const double* notional, const double* spread, const double* fix_sign,
                                 const double* flt_sign, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv,
                                 int n_threads);
int adr_scenario_subbook_var_es(adr_ctx* ctx, int interp_method, int K, const double* times, int S, const double* dfs,
                                const adr_trades* trades, int64_t B, const int64_t* sub_off, int base_col, int k, double* var,
                                double* es);
int adr_credit_scenario_subbook_pv(adr_ctx* ctx, int interp_method, int K, const double* times, int S_disc, const double* dfs,
                                   int G, int S_spr, const double* dz, int S, const adr_trades* trades, const double* z,
                                   const int32_t* bucket, int64_t n_fix, const double* fix_tau, int64_t n_flt,
                                   const double* flt_tau, int64_t B, const int64_t* sub_off, double* pv, double* sub_pv);
int adr_credit_scenario_subbook_pv_set(adr_ctx* ctx, const adr_curve_set* set, int G, int S_spr, const double* dz,
                                       const adr_trades* trades, const double* z, const int32_t* bucket, int64_t n_fix,
                                       const double* fix_tau, int64_t n_flt, const double* flt_tau, int64_t B,
                                       const int64_t* sub_off, double* pv, double* sub_pv);
int adr_credit_scenario_subbook_pv_dev(adr_ctx* ctx, int interp_method, int K, const double* times_dev, int S_disc,
                                       const double* dfs_dev, int G, int S_spr, const double* dz_dev, int S,
                                       const adr_trades* trades, const double* z_dev, const int32_t* bucket_dev, int64_t n_fix,
                                       const double* fix_tau_dev, int64_t n_flt, const double* flt_tau_dev, int64_t B,
                                       const int64_t* plan_dev, double* pv_dev, double* sub_pv_dev, double* work_dev, void* stream);
int adr_credit_scenario_subbook_pv_host(int interp_method, int K, const double* times, int S_disc, const double* dfs, int G,
                                        int S_spr, const double* dz, int S, int64_t n, const int64_t* fix_off,
                                        const int64_t* flt_off, const double* fix_tp, const double* fix_pay, const double* flt_tp,
                                        const double* flt_ts, const double* flt_te, const double* flt_alpha,
                                        const double* flt_weight, const double* notional, const double* spread,
                                        const double* fix_sign, const double* flt_sign, const double* z, const int32_t* bucket,
                                        const double* fix_tau, const double* flt_tau, int64_t B, const int64_t* sub_off,
                                        double* pv, double* sub_pv, int n_threads);

/*
 * Tail measures of B rows at once: historical-simulation VaR and expected shortfall per sub-book.  rows[B][S_tot];
 * base_col >= 0: the P&L of row b is rows[b][s] - rows[b][base_col] for every OTHER column s (the base curve priced as
 * one more scenario); base_col = -1: the rows already are P&L.  k = 1 .. the P&L values per row.  var[b] is minus the
 * k-th smallest P&L; es[b] is minus the sum of the k smallest, added in ascending order from 0.0, divided by k.  A row
 * holding a NaN gives NaN in both.  No interpolation between order statistics.  One block per row sorts the row in LDS
 * (a bitonic network over the next power of two, padded with +inf); rows of more than ADR_SCENARIO_TAIL_MAX P&L values
 * are ADR_ERR_UNSUPPORTED.  adr_scenario_tail: host arrays, blocks; _dev: device arrays on `stream`, no allocation, no
 * synchronisation; _host: the CPU twin, the same sums in the same order, hence the same bits.
 */
#define ADR_SCENARIO_TAIL_MAX 16384
int adr_scenario_tail(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es);
int adr_scenario_tail_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k, double* var_dev,
                          double* es_dev, void* stream);
int adr_scenario_tail_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es);

/*
 * YoY sub-books: adr_yoy_scenario_pv* per sub-book in one launch.  The entries take what adr_yoy_scenario_pv* take plus
 * B >= 1, sub_off[B + 1] (sub-book b holds the swaps sub_off[b] .. sub_off[b + 1]; from 0 to n, not decreasing, empty
 * sub-books allowed) and sub_pv[B][S], under the contract of the sub-book entries above, word for word: sub_pv[b][s]
 * has exactly the bits of adr_yoy_scenario_pv's book_pv[s] on a batch holding sub-book b's swaps alone - chunks of 64
 * swaps from sub_off[b], the sub-book's chunk j to slot j % 64 in order, then the halving tree, no atomics; an empty
 * sub-book gives +0.0; a row does not depend on B, on the other sub-books, on S or on whether the discount table is in
 * LDS; pv[n][S], when given, has the parent's bits.  The blocking and the _host entries check the offsets
 * (ADR_ERR_INVALID naming the sub-book) and build the plan themselves.  The _dev entry takes the uploaded plan of
 * adr_scenario_subbook_plan and adr_scenario_subbook_work(n, B, S) doubles of scratch, enqueues three kernels on
 * `stream` without allocation or synchronisation and checks scalars only: a plan whose bounds leave 0 .. n is cut to
 * that range, one with more chunks than the scratch holds is cut there.
 */
int adr_yoy_scenario_subbook_pv(adr_ctx* ctx, int disc_method, int K, const double* times, int S_disc, const double* dfs,
                                int infl_method, int P, const double* T, int S_infl, const double* b, int S, int64_t n,
                                int64_t n_fix, const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                                const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, double* pv,
                                double* sub_pv);
int adr_yoy_scenario_subbook_pv_dev(adr_ctx* ctx, int disc_method, int K, const double* times_dev, int S_disc,
                                    const double* dfs_dev, int infl_method, int P, const double* T_dev, int S_infl,
                                    const double* b_dev, int S, int64_t n, int64_t n_fix, const int64_t* fix_off_dev,
                                    const double* fix_tp_dev, const double* fix_pay_dev, int64_t m, const int64_t* cpn_off_dev,
                                    const double* cpn_dev, int64_t B, const int64_t* plan_dev, double* pv_dev, double* sub_pv_dev,
                                    double* work_dev, void* stream);
int adr_yoy_scenario_subbook_pv_host(int disc_method, int K, const double* times, int S_disc, const double* dfs, int infl_method,
                                     int P, const double* T, int S_infl, const double* b, int S, int64_t n, int64_t n_fix,
                                     const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                                     const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, double* pv,
                                     double* sub_pv, int n_threads);

/*
 * Tail allocation: how much of the FIRM's VaR and expected shortfall each row (desk) carries - the Euler allocation, the
 * one that adds up to the firm's figure.  rows[B][S_tot], base_col and k as in adr_scenario_tail; pnl[b][e] is P&L value
 * e of row b (every other column minus base_col, or the row itself when base_col = -1).
 *
 *   tot[e]  = sum_b pnl[b][e] in a fixed order: row b to slot b % 64, each slot added in row order from 0.0, then slots
 *             0-31 += 32-63, ..., 0 += 1.
 *   e_1 ..  = the scenarios ordered by (key(tot[e]), e) ascending: adr_scenario_tail's total order of the doubles
 *             (-0.0 before +0.0), ties to the lower scenario index.
 *   var_tot = -tot[e_k];       es_tot     = -(tot[e_1] + .. + tot[e_k]) / k, added in that order from 0.0
 *   comp_var[b] = -pnl[b][e_k]; comp_es[b] = -(pnl[b][e_1] + .. + pnl[b][e_k]) / k, in the same order from 0.0
 *
 * If any tot[e] is NaN every output is NaN.  var_tot and es_tot are adr_scenario_tail's var and es of the one-row matrix
 * tot, bit for bit; sum_b comp_es[b] = es_tot and sum_b comp_var[b] = var_tot up to the rounding of the sums.  No
 * atomics, no interpolation.  The ordering is a bitonic network over (key, index) pairs of 16 bytes in LDS, so rows of
 * more than ADR_SCENARIO_ALLOC_MAX P&L values are ADR_ERR_UNSUPPORTED.  adr_scenario_tail_alloc: host arrays, blocks;
 * _dev: device arrays on `stream` (NULL: the ctx's own), work_dev holds S_tot doubles, no allocation and no
 * synchronisation (three kernels in one chain); _host: the CPU twin, the same sums in the same order, hence the same
 * bits.
 */
#define ADR_SCENARIO_ALLOC_MAX 8192
int adr_scenario_tail_alloc(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot,
                            double* es_tot, double* comp_var, double* comp_es);
int adr_scenario_tail_alloc_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k,
                                double* var_tot_dev, double* es_tot_dev, double* comp_var_dev, double* comp_es_dev,
                                double* work_dev, void* stream);
int adr_scenario_tail_alloc_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot, double* es_tot,
                                 double* comp_var, double* comp_es);

/*
 * Sub-book Greeks: the PV, delta and gamma ladders of every sub-book of a batch on one curve from one launch chain -
 * what one aggregate-only adr_price per desk returns, without the loop.  B >= 1 and sub_off[B + 1] as for the scenario
 * sub-books above (from 0 to n, not decreasing, empty sub-books allowed).  out[B][1 + P + P * P], row-major, is
 * adr_price's agg per sub-book: [pv, delta[P], gamma[P][P]]; pv always, delta with ADR_REQ_DELTA or ADR_REQ_GAMMA, gamma
 * with ADR_REQ_GAMMA, the blocks not requested are zeros.  The entries write and do not add.
 *
 * The batch is read from its CSR arrays in chunks of ADR_SCENARIO_CHUNK trades cut at sub-book boundaries (the plan of
 * adr_scenario_subbook_plan).  A chunk's knot-space record [pv, w[Kc], D[Kc], O[Kc]] (without GAMMA: [pv, w[Kc]])
 * depends on its trades alone; a sub-book's records are added in the plan's order (chunk j to slot j % 64 in order,
 * then slots 0-31 += 32-63, ..., 0 += 1; no atomics to global memory) and projected once per sub-book.  So a
 * sub-book's row has exactly the bits of the same entry called with B = 1 on a batch holding its trades alone, does not
 * depend on B or on the other sub-books, and is bit-identical from run to run; an empty sub-book's row is +0.0.
 *
 * Covered: every trade without ratio nodes - no per-coupon notional other than 1 and every accruing float coupon paid
 * on its accrual end (bonds, single-curve FRNs, OIS without payment lag) -, the three interpolation schemes, any pillar
 * count the curve handle carries.  A batch that holds a ratio node is ADR_ERR_UNSUPPORTED, naming the first such trade;
 * so is a curve whose knot tables for one wave (24 Kc bytes with GAMMA) do not fit the LDS.
 *
 * adr_subbook_ladders: host out, blocks.  _dev: device out and scratch, the uploaded plan, enqueues on `stream` (NULL:
 * the ctx's own) without allocation or synchronisation (knot sums, the sum for small and for large sub-books, the
 * projection) and checks scalars only, cutting the plan as the scenario _dev entries do.  adr_subbook_ladders_work is
 * its scratch in doubles, (ceil(n / 64) + 2 B) records, and leaves the rows of chunk records that scratch holds in
 * *chunks when that is not NULL.  _host: the CPU twin on the curve's (times, dfs, jac, hess) as adr_curve_upload takes
 * them (hess may be NULL without GAMMA) and a TradeBatch's arrays: the same node and projection code, chunks and
 * summation orders; it differs from the device by the two exp implementations only.
 */
/* flags[i] = 1 where trade i has a ratio node (the rule adr_trades_upload applies), else 0; flt_weight may be NULL. */
int adr_trades_ratio_flags_host(int64_t n, const int64_t* flt_off, const double* flt_tp, const double* flt_te,
                                const double* flt_alpha, const double* flt_weight, uint8_t* flags);
int64_t adr_subbook_ladders_work(const adr_curve* curve, int64_t n, int64_t B, uint32_t req_mask, int64_t* chunks);
int adr_subbook_ladders(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, int64_t B, const int64_t* sub_off,
                        uint32_t req_mask, double* out);
int adr_subbook_ladders_dev(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, int64_t B, const int64_t* plan_dev,
                            uint32_t req_mask, double* out_dev, double* work_dev, void* stream);
int adr_subbook_ladders_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac,
                             const double* hess, int64_t n, const int64_t* fix_off, const int64_t* flt_off, const double* fix_tp,
                             const double* fix_pay, const double* flt_tp, const double* flt_ts, const double* flt_te,
                             const double* flt_alpha, const double* flt_weight, const double* notional, const double* spread,
                             const double* fix_sign, const double* flt_sign, int64_t B, const int64_t* sub_off, uint32_t req_mask,
                             double* out);

/*
 * Delta-gamma P&L of ladders under a scenario set: what the rows of adr_subbook_ladders* (or adr_price's agg) say a desk
 * makes when the par quotes move, without a revaluation.  ladders[B][1 + P + P * P] has exactly that layout - pv,
 * delta[P] per bp, gamma[P][P] per bp^2, row-major -; the pv slot is not read, and gamma is used as given (no symmetry is
 * assumed).  shocks_bp[S][P]: shocks_bp[s][p] is scenario s's move of par quote p in basis points.  Outputs [B][S] each:
 *
 *   pnl_delta[b][s] = sum_p delta_p x_p
 *   pnl_gamma[b][s] = 1/2 sum_p sum_q gamma_pq x_p x_q
 *   pnl[b][s]       = pnl_delta[b][s] + pnl_gamma[b][s]
 *
 * Any of the three may be NULL (at least one is asked for); an output not asked for is not touched.  Every step is one
 * fused multiply-add, rounded once, in this order (x = shocks_bp[s], the row b of ladders):
 *
 *   dl  = fma(delta_p, x_p, dl)       p = 0 .. P - 1 ascending, from +0.0
 *   t_p = fma(gamma_pq, x_q, t_p)     q = 0 .. P - 1 ascending, from +0.0, for every row p of gamma
 *   gm  = fma(t_p, x_p, gm)           p = 0 .. P - 1 ascending, from +0.0
 *   pnl_delta = dl,   pnl_gamma = 0.5 * gm (exact),   pnl = dl + 0.5 * gm
 *
 * so pnl == pnl_delta + pnl_gamma bit for bit.  There is no exp, no atomic and no sum across lanes: the device and the
 * host twin agree BIT FOR BIT, and pnl[b][s] depends on ladder row b and shock row s alone - not on B, S, the position
 * of either row, or the run.  A NaN in row b makes pnl[b][.] NaN and touches no other row.  With only pnl_delta asked
 * for gamma is not read.
 *
 * B >= 0 (B = 0 writes nothing and succeeds; ladders may then be NULL), S >= 1 (at most 65535 * 64 on the device),
 * 1 <= P <= ADR_LADDER_PNL_MAX_PILLARS - beyond that ADR_ERR_UNSUPPORTED: the shocks of 64 scenarios sit in the LDS of a
 * CU, 512 P bytes.  Bad scalars, a NULL input or no output: ADR_ERR_INVALID.  adr_ladder_pnl: host arrays, blocks (one
 * allocation); _dev: device arrays, one kernel on `stream` (NULL: the ctx's own), no allocation, no synchronisation,
 * scalar checks only; _host: the CPU twin, the same expression per element.
 */
#define ADR_LADDER_PNL_MAX_PILLARS 256
int adr_ladder_pnl(adr_ctx* ctx, int64_t B, int P, const double* ladders, int S, const double* shocks_bp, double* pnl,
                   double* pnl_delta, double* pnl_gamma);
int adr_ladder_pnl_dev(adr_ctx* ctx, int64_t B, int P, const double* ladders_dev, int S, const double* shocks_bp_dev,
                       double* pnl_dev, double* pnl_delta_dev, double* pnl_gamma_dev, void* stream);
int adr_ladder_pnl_host(int64_t B, int P, const double* ladders, int S, const double* shocks_bp, double* pnl, double* pnl_delta,
                        double* pnl_gamma);

/*
 * Correlated normal shocks from a factor matrix: the scenario set of a Monte Carlo delta-gamma VaR, made where
 * adr_ladder_pnl* reads it.  factor[P][F], row-major, 1 <= F <= P <= ADR_LADDER_PNL_MAX_PILLARS: a Cholesky factor of the
 * covariance of the quote moves in bp^2, or fewer PCA columns.  out[S][P], adr_ladder_pnl's shocks_bp:
 *
 *   out[s][p] = sum_j factor[p][j] z[s][j]                                        (basis points)
 *
 * Row s is GLOBAL row first_scenario + s (first_scenario >= 0), so a set can be made in pieces.  Its normals belong to the
 * generating scenario g: g = the global row, or with antithetic = 1 the global row >> 1, and then the odd global rows are
 * the exact negation (sign bit flipped, zeros included) of the even rows before them.
 *
 *   generator  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key
 *              (seed lo, seed hi), counter (g lo, g hi, j / 2, 0); one call yields the words w0 .. w3
 *   uniforms   u1 = (((w1 << 32 | w0) >> 11) + 0.5) * 2^-53, u2 the same from w3, w2: the 53-bit integer is exact, the sum
 *              is rounded once to nearest even and the scaling is exact, so u lies in (0, 1] - 1.0 when all 53 bits are
 *              set - and is never 0: there is no log(0)
 *   normals    r = sqrt(-2 log(u1)); z[2 (j / 2)] = r cos(2 pi u2), z[2 (j / 2) + 1] = r sin(2 pi u2), 2 pi the nearest
 *              double; an odd F drops the last sine
 *   products   x = fma(factor[p][j], z_j, x) for j = 0 .. F - 1 ascending, from +0.0; the antithetic negation comes last
 *
 * A row depends on seed, its global index, factor and antithetic alone: not on S, on how first_scenario splits the set,
 * on the launch geometry or on the run.  u has the same bits on the device and in the host twin; log, sqrt, cos and sin
 * are each side's library, so z and out agree to a few ulp of their terms, not bit for bit.  Refused with
 * ADR_ERR_INVALID: F > P, P > ADR_LADDER_PNL_MAX_PILLARS, S < 1, F < 1, first_scenario < 0 (or first_scenario + S beyond
 * an int64), antithetic other than 0 / 1, NULL pointers.  adr_shock_normal: host arrays, blocks (one allocation); _dev:
 * device arrays, one kernel on `stream` (NULL: the ctx's own), no allocation, no synchronisation, scalar checks only;
 * _host: the CPU twin, the same code.
 *
 * Test hooks: adr_shock_words_host is the raw Philox4x32-10 block of a counter and a key; adr_shock_uniforms* write
 * u[S][ceil(F / 2)][2], (u1, u2) of every pair of every row, from the host twin and from the device (host arrays, blocks).
 */
int adr_shock_normal(adr_ctx* ctx, uint64_t seed, int64_t first_scenario, int S, int P, int F, const double* factor, int antithetic,
                     double* out);
int adr_shock_normal_dev(adr_ctx* ctx, uint64_t seed, int64_t first_scenario, int S, int P, int F, const double* factor_dev,
                         int antithetic, double* out_dev, void* stream);
int adr_shock_normal_host(uint64_t seed, int64_t first_scenario, int S, int P, int F, const double* factor, int antithetic,
                          double* out);
void adr_shock_words_host(const uint32_t counter[4], const uint32_t key[2], uint32_t words[4]);
int adr_shock_uniforms(adr_ctx* ctx, uint64_t seed, int64_t first_scenario, int S, int F, int antithetic, double* u);
int adr_shock_uniforms_host(uint64_t seed, int64_t first_scenario, int S, int F, int antithetic, double* u);

/*
 * adr_scenario_tail for rows of any width: var[b] and es[b] of rows[B][S_tot] by adr_scenario_tail's definition, word for
 * word - base_col, k, var[b] minus the k-th smallest P&L, es[b] minus the sum of the k smallest added in ascending order
 * from 0.0 and divided by k, the total order of the doubles (-0.0 before +0.0), NaN in both for a row holding a NaN.  The
 * limit is on the tail, not on the row: 1 <= k <= ADR_SCENARIO_TAIL_MAX (beyond: ADR_ERR_UNSUPPORTED); the P&L values per
 * row are bounded by int alone.  k < 1, k beyond the P&L values per row, a bad base_col, B < 1, NULL arrays:
 * ADR_ERR_INVALID.  For rows adr_scenario_tail takes the results have its bits.
 *
 * Device: a radix select on the 64-bit keys, 11 bits a round from the top (six rounds: a histogram kernel over
 * (segment, row) blocks with integer LDS atomics and a scan kernel per row), a gather of the values below the k-th into
 * tail[B][k], padded with the k-th value itself, then adr_scenario_tail's kernel on that matrix.  Only integer atomics,
 * whose sums do not depend on the order of arrival; the kernel boundary is the only synchronisation; two runs give the
 * same bits.  adr_scenario_tail_select: host arrays, blocks (one allocation); _dev: device arrays and work_dev -
 * adr_scenario_tail_select_work(B, S_tot, k) bytes, 16-byte aligned, contents free - on `stream`, no allocation, no
 * synchronisation; _host: the CPU twin - std::nth_element on the keys, a sort of the k smallest, the same sum - the same
 * bits.  adr_scenario_tail_select_work returns 0 for sizes the entries refuse.
 */
int adr_scenario_tail_select(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es);
int adr_scenario_tail_select_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k, double* var_dev,
                                 double* es_dev, void* work_dev, void* stream);
int adr_scenario_tail_select_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var, double* es);
int64_t adr_scenario_tail_select_work(int64_t B, int S_tot, int k);

/*
 * The ordered tail select: a row's k worst scenarios as INDICES, in the row's order - what the tail allocation needs of
 * the firm's P&L.  rows[B][S_tot], base_col and k are read as adr_scenario_tail_select reads them; pnl[b][e] is P&L value
 * e of row b.  The scenarios of a row are ordered by (key(pnl[b][e]), e) ascending: adr_scenario_tail's total order of
 * the doubles (-0.0 before +0.0), ties to the lower scenario index - adr_scenario_tail_alloc's rule.  With e_1, e_2, ..
 * that order:
 *
 *   order[b][0 .. k-1] = e_1 .. e_k   int64, P&L indices: the base column is not counted, as in adr_scenario_tail_alloc
 *   var[b] = -pnl[b][e_k];   es[b] = -(pnl[b][e_1] + .. + pnl[b][e_k]) / k, added in that order from 0.0
 *
 * so var and es have adr_scenario_tail_select's bits.  A row holding a NaN gives var = es = NaN and order[b][.] = -1, and
 * touches no other row.  1 <= k <= ADR_SCENARIO_ALLOC_MAX (k pairs of 16 bytes are sorted in LDS); a larger k is
 * ADR_ERR_UNSUPPORTED, the other refusals are adr_scenario_tail_select's; the row may have any width.
 *
 * Device: adr_scenario_tail_select's six count / scan rounds find the k-th key; a gather then writes (key, index) pairs.
 * Pairs below the k-th key take any slot.  Of the pairs EQUAL to it exactly the k_rem with the lowest indices are taken,
 * by rank: the ties of earlier segments (the last round's histograms), of earlier 256-element chunks of the block (a
 * running count) and of lower lanes (ballot and popcount); rank r < k_rem goes to slot below + r.  What is selected
 * depends on no atomic's return value and not on the order in which blocks and waves arrive.  One block per row then
 * sorts the k pairs (adr_scenario_tail_alloc's bitonic network, padded with +inf) and writes order, var and es.  Only
 * integer atomics; the kernel boundary is the only synchronisation; two runs give the same bits.
 * adr_scenario_tail_order: host arrays, blocks (one allocation); _dev: device arrays and work_dev -
 * adr_scenario_tail_order_work(B, S_tot, k) bytes, 16-byte aligned, contents free - on `stream` (NULL: the ctx's own), no
 * allocation, no synchronisation; _host: the CPU twin - std::nth_element on the pairs, a sort of the first k, the same
 * sums - the same bits.  adr_scenario_tail_order_work returns 0 for sizes the entries refuse.
 */
int adr_scenario_tail_order(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, int64_t* order, double* var,
                            double* es);
int adr_scenario_tail_order_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k, int64_t* order_dev,
                                double* var_dev, double* es_dev, void* work_dev, void* stream);
int adr_scenario_tail_order_host(int64_t B, int S_tot, const double* rows, int base_col, int k, int64_t* order, double* var, double* es);
int64_t adr_scenario_tail_order_work(int64_t B, int S_tot, int k);

/*
 * adr_scenario_tail_alloc for a matrix of any width: the same outputs, the same sums in the same order, NaN everywhere
 * when a total is NaN.  The limit moves from the row to the tail: 1 <= k <= ADR_SCENARIO_ALLOC_MAX, beyond that
 * ADR_ERR_UNSUPPORTED; the other refusals are adr_scenario_tail_alloc's.  Where adr_scenario_tail_alloc takes the rows the
 * results have its bits.  Device: its column-sum kernel, adr_scenario_tail_order on the one-row tot, its components
 * kernel.  adr_scenario_tail_alloc_select: host arrays, blocks (one allocation); _dev: device arrays and work_dev -
 * adr_scenario_tail_alloc_select_work(B, S_tot, k) bytes, 16-byte aligned - on `stream`, no allocation, no
 * synchronisation; _host: the CPU twin, the same bits.  _work returns 0 for sizes the entries refuse.
 *
 * adr_scenario_total*: tot[e] alone, m values (S_tot, or S_tot - 1 with a base column) - the fixed-order column sums of
 * adr_scenario_tail_alloc.  On ladder rows [B][1 + P + P P] with base_col = -1 it is the firm's ladder row.
 */
int adr_scenario_tail_alloc_select(adr_ctx* ctx, int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot,
                                   double* es_tot, double* comp_var, double* comp_es);
int adr_scenario_tail_alloc_select_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, int k,
                                       double* var_tot_dev, double* es_tot_dev, double* comp_var_dev, double* comp_es_dev,
                                       void* work_dev, void* stream);
int adr_scenario_tail_alloc_select_host(int64_t B, int S_tot, const double* rows, int base_col, int k, double* var_tot, double* es_tot,
                                        double* comp_var, double* comp_es);
int64_t adr_scenario_tail_alloc_select_work(int64_t B, int S_tot, int k);
int adr_scenario_total_dev(adr_ctx* ctx, int64_t B, int S_tot, const double* rows_dev, int base_col, double* tot_dev, void* stream);
int adr_scenario_total_host(int64_t B, int S_tot, const double* rows, int base_col, double* tot);

/*
 * The two steps between the firm's order and the desks' components in a Monte Carlo tail allocation (delta-gamma P&L is
 * linear in the ladder row: the firm's P&L is adr_ladder_pnl of the sum of the desks' rows, and a desk is priced at the
 * firm's k worst shocks alone).
 *
 * adr_shock_gather*: out[i][p] = shocks[order[i]][p] for i < k; shocks[S][P], order[k] as adr_scenario_tail_order writes
 * it.  When order[0] is negative (the firm's row held a NaN) every out value is NaN, and so is row i when order[i] is
 * no row of shocks: adr_ladder_pnl* then turns every desk's figures into NaN without a host round trip.  k >= 1, S >= 1,
 * 1 <= P <= ADR_LADDER_PNL_MAX_PILLARS, else ADR_ERR_INVALID.
 *
 * adr_tail_components*: pnl[B][k] holds every row's P&L at the firm's k worst scenarios, in the firm's order:
 *   comp_es[b] = -(pnl[b][0] + .. + pnl[b][k-1]) / k, added in that order from 0.0;   comp_var[b] = -pnl[b][k-1]
 * - adr_scenario_tail_alloc's component sums, so on the gathered columns of a matrix they have its bits.  B >= 1, k >= 1.
 *
 * _dev: device arrays, one kernel on `stream` (NULL: the ctx's own), no allocation, no synchronisation, scalar checks
 * only; _host: the CPU twin, the same bits.
 */
int adr_shock_gather_dev(adr_ctx* ctx, int k, int P, const double* shocks_dev, int S, const int64_t* order_dev, double* out_dev,
                         void* stream);
int adr_shock_gather_host(int k, int P, const double* shocks, int S, const int64_t* order, double* out);
int adr_tail_components_dev(adr_ctx* ctx, int64_t B, int k, const double* pnl_dev, double* comp_var_dev, double* comp_es_dev,
                            void* stream);
int adr_tail_components_host(int64_t B, int k, const double* pnl, double* comp_var, double* comp_es);

/*
 * Discount factors of shocked curves, values only: the link between the Monte Carlo shock rows and the scenario kernels,
 * which read discount factors alone.  For shock row s of shocks_bp[S][ld] (basis points; the first P columns are read,
 * ld >= P is the row stride, so augmented rows - spread or breakeven columns behind the quotes - go in without a copy):
 *
 *   r_p  = base_rates[p] + shocks_bp[s][p] * 1e-4           (one rounded product, one rounded sum)
 *   v    = 1 + r a_i ;  Pp = 0 <= prev_idx[i] < i ? pv01[prev_idx[i]] : 0 ;  r = r_{pillar[i]}
 *   d_i  = prev_idx[i] >= 0 ? (1 - r Pp) / v : 1 / v ;  pv01[i] = Pp + a_i d_i ;  dfs[s][i] = d_i       i = 0 .. K - 1
 *
 * - the scan of adr_curve_set_build without its Jacobian and Hessian: 8 K bytes per scenario instead of
 * 8 K (1 + P + P P).  Every step is one IEEE operation in this order, nothing is fused and no library function is
 * called: dfs[s] has the bits of adr_curve_set_build's discount factors at the rates r, on the device and on the host.
 * bad[s] (NULL: not wanted) is 1 where any d_i of scenario s is not finite or not positive, else 0; the row is written
 * all the same.
 *
 * adr_curve_dfs_shocked_dev: `plan`'s scan arrays (acc, pillar, prev_idx; K knots, P <= ADR_MAX_PLAN_PILLARS pillars),
 * device arrays, and work_dev of adr_curve_dfs_shocked_work(plan, S) DOUBLES, (K + P) S: one kernel on `stream` (NULL:
 * the ctx's own), no allocation, no synchronisation, scalar checks only.  adr_curve_dfs_shocked: host arrays, blocks (one
 * allocation); it also refuses base rates that are not finite.  adr_curve_dfs_shocked_host: the CPU twin on the scan
 * arrays themselves, no GPU and no plan; it also refuses a pillar outside 0 .. P - 1 and a prev_idx outside -1 .. K - 1.
 * ADR_ERR_INVALID: NULL pointers (bad excepted), S < 1, ld < P, a plan of another ctx.  _work returns 0 for those.
 *
 * adr_scenario_rows_place_dev: rows[b][s0 + s] = tile[b][s] for b < B, s < S_tile; tile[B][S_tile], rows[B][S_tot].  The
 * sub-book launch writes [B][S_tile] for a tile of scenarios, the tail entries read rows [B][S_tot].  One kernel on
 * `stream`.  ADR_ERR_INVALID: B < 1, S_tile < 1, s0 < 0, s0 + S_tile > S_tot, NULL pointers.
 */
int adr_curve_dfs_shocked(adr_ctx* ctx, const adr_curve_plan* plan, const double* base_rates, int S, int ld, const double* shocks_bp,
                          double* dfs, int32_t* bad);
int adr_curve_dfs_shocked_dev(adr_ctx* ctx, const adr_curve_plan* plan, const double* base_rates_dev, int S, int ld,
                              const double* shocks_bp_dev, double* dfs_dev, int32_t* bad_dev, double* work_dev, void* stream);
int64_t adr_curve_dfs_shocked_work(const adr_curve_plan* plan, int S);
int adr_curve_dfs_shocked_host(int K, int P, const double* acc, const int32_t* pillar, const int32_t* prev_idx, const double* base_rates,
                               int S, int ld, const double* shocks_bp, double* dfs, int32_t* bad);
int adr_scenario_rows_place_dev(adr_ctx* ctx, int64_t B, int S_tile, const double* tile_dev, int S_tot, int s0, double* rows_dev,
                                void* stream);

/*
 * Columns of the joint shock rows as the credit and inflation scenario kernels read them, and the three product lines'
 * sub-book rows in one matrix: what full revaluation of a firm needs between adr_shock_normal_dev, the sub-book launches
 * and the tail entries, on the device.
 *
 * adr_shock_columns*: shocks_bp[S][ld] in basis points, one joint row per scenario (quotes, then spread buckets, then
 * breakevens); columns col0 .. col0 + n of every row become the dense out[S][n]:
 *
 *   out[s][j] = base[j] + shocks_bp[s][col0 + j] * 1e-4     (base NULL: the product itself, so -0.0 stays -0.0)
 *
 * - one rounded product, then one rounded sum, never fused: the bits of NumPy's b0 + x * 1e-4 (`shocked_breakevens`) and
 * of x * 1e-4 (`shocked_spreads`), on the device and on the host.  base NULL gives dz[S][G] in decimals for
 * adr_credit_scenario_subbook_pv_dev, base = the curve's breakeven rates gives b[S][P_i] for
 * adr_yoy_scenario_subbook_pv_dev.  bad[s] (NULL: not wanted) is set to 1 where any out[s][j] is not finite or, with
 * floor_on != 0, is <= floor (breakevens: floor = -1.0, where 1 + b <= 0 has no inflation factor), and is LEFT AS IT IS
 * otherwise: the entry chains behind adr_curve_dfs_shocked_dev on one array of flags.  The row is written all the same.
 * No atomics: every lane that finds a bad entry stores the constant 1.
 *
 * _dev: device arrays, one kernel on `stream` (NULL: the ctx's own), no allocation, no synchronisation, 64-bit indices,
 * scalar checks only.  adr_shock_columns: host arrays, blocks (one allocation); bad goes in and comes back.  _host: the
 * CPU twin, the same bits.  ADR_ERR_INVALID: S < 1, n < 1, col0 < 0, ld < col0 + n, NULL shocks_bp or out.
 *
 * adr_scenario_rows_merge*: tile[B][S_tile] into rows[B_tot][S_tot] through a row map,
 *
 *   rows[target[b]][s0 + s] = tile[b][s]                            where add == NULL or add[b] == 0
 *   rows[target[b]][s0 + s] = rows[target[b]][s0 + s] + tile[b][s]  otherwise
 *
 * for b < B and s < S_tile; a target outside 0 .. B_tot - 1 skips its row; nothing else of rows is touched.  The targets
 * of one call must be distinct: the caller's duty for _dev, refused by _host (ADR_ERR_INVALID naming the row).  Calls on
 * one stream are ordered, so with one call per product line a desk's row is its first line's row with the later lines'
 * rows added in line order.  _dev: one kernel on `stream`, no allocation, no synchronisation, no atomics.
 * ADR_ERR_INVALID: B < 1, S_tile < 1, B_tot < 1, S_tot < 1, s0 < 0, s0 + S_tile > S_tot, NULL tile, rows or target.
 */
int adr_shock_columns(adr_ctx* ctx, int S, int ld, const double* shocks_bp, int col0, int n, const double* base, int floor_on, double floor,
                      double* out, int32_t* bad);
int adr_shock_columns_dev(adr_ctx* ctx, int S, int ld, const double* shocks_bp_dev, int col0, int n, const double* base_dev, int floor_on,
                          double floor, double* out_dev, int32_t* bad_dev, void* stream);
int adr_shock_columns_host(int S, int ld, const double* shocks_bp, int col0, int n, const double* base, int floor_on, double floor,
                           double* out, int32_t* bad);
int adr_scenario_rows_merge_dev(adr_ctx* ctx, int64_t B, int S_tile, const double* tile_dev, int64_t B_tot, int S_tot, int s0,
                                double* rows_dev, const int64_t* target_dev, const int32_t* add_dev, void* stream);
int adr_scenario_rows_merge_host(int64_t B, int S_tile, const double* tile, int64_t B_tot, int S_tot, int s0, double* rows,
                                 const int64_t* target, const int32_t* add);

/*
 * Credit sub-book Greeks: per sub-book the PV, the curve delta and gamma AT THE TRADES' SPREADS, CS01 and spread gamma
 * per credit bucket and the rate x spread cross gamma, from one launch chain.  The spread side is adr_credit_scenario_pv's:
 * z[n] (z-spread of a bond, discount margin of an FRN), bucket[n] in -1 .. G - 1 (-1: no bucket), 0 <= G <=
 * ADR_CREDIT_MAX_BUCKETS, and one spread time per fixed flow / float coupon (fix_tau[n_fix], flt_tau[n_flt]); every
 * payment is discounted at D(tp) exp(-z tau), the forward carries no spread.  The batch must be ordered by (sub-book,
 * bucket): inside a sub-book the buckets do not decrease (unbucketed trades first).  A (sub-book, bucket) pair that holds
 * trades is a CELL; C <= min(n, B (G + 1)) cells exist.
 *
 * out[B][1 + Q + Q * Q], Q = P + G, row-major, is an AUGMENTED ladder in agg's layout with Q in place of P:
 *
 *   out[b][0]                           pv of sub-book b at its spreads
 *   delta'[p < P]                       curve delta per bp, at the spreads
 *   delta'[P + g]                       CS01: dPV / dz of the sub-book's trades of bucket g, per bp
 *   gamma'[p][q], p, q < P              curve gamma per bp^2, at the spreads
 *   gamma'[p][P + g] = gamma'[P + g][p] d2PV / dz dquote_p of cell (b, g), per bp^2: ONE value stored twice
 *   gamma'[P + g][P + g]                d2PV / dz^2 of cell (b, g), per bp^2
 *   everything else                     +0.0 (a trade has one bucket: the spread-spread block is diagonal)
 *
 * so adr_ladder_pnl* with P := Q and shock rows [x_bp[P], dz * 1e4 [G]] gives the joint second-order expansion
 * delta . x + x' Gamma x / 2 + sum_g (cs01_g y_g + csg_g y_g^2 / 2 + y_g cross_g . x), and adr_scenario_tail* apply to the
 * result as they stand (Q <= ADR_LADDER_PNL_MAX_PILLARS is a limit of that step, not of these entries).  A sub-book
 * without bucket g has +0.0 there; unbucketed trades are priced at their z and enter the curve block only.  pv always,
 * delta' with ADR_REQ_DELTA or ADR_REQ_GAMMA, gamma' with ADR_REQ_GAMMA; blocks not requested are zeros.  The entries write
 * and do not add.
 *
 * A chunk (at most ADR_SCENARIO_CHUNK trades of ONE cell) gives the record [pv, w[Kc], D[Kc], O[Kc], wz[Kc], cs, csg]
 * (without GAMMA [pv, w[Kc], cs]); a cell's records are added in the plan's order by adr_subbook_ladders' rule, and by
 * the same rule a sub-book's cell sums (cell j of the sub-book to slot j % 64, then the halving tree).  The curve block is
 * projected from the sub-book's sums, the spread rows and columns from the cells' sums.  Contract: a sub-book's row has
 * exactly the bits of the same entry called with B = 1 on that sub-book's trades alone with the same buckets and G - on
 * the host twin and on the device -, does not depend on B or on the other sub-books, and repeats bit for bit from run to
 * run; an empty sub-book's row is +0.0 throughout; gamma' is symmetric bit for bit in its cross rows and columns.  The
 * device part rests on the same observed ordering of the LDS adds (ds_add_f64) as adr_subbook_ladders.  On the host twin,
 * z = 0 everywhere and G = 0 give adr_subbook_ladders_host's rows bit for bit; on the device the rows agree with
 * adr_subbook_ladders' to rounding only (the two knot kernels are different programs).  A trade with z == 0 has the
 * factor 1.0 exactly, whatever its spread times hold.
 *
 * Refused: a ratio node (ADR_ERR_UNSUPPORTED, adr_subbook_ladders' wording), a curve whose tables for one wave (32 Kc
 * bytes with GAMMA, 8 Kc without) do not fit the LDS (ADR_ERR_UNSUPPORTED); by the blocking entry and the host twin also
 * what they can read: non-finite z or spread times, a bucket outside -1 .. G - 1, G outside 0 .. ADR_CREDIT_MAX_BUCKETS,
 * a sub-book whose trades are not ordered by bucket (ADR_ERR_INVALID, naming the trade).  _dev checks scalars only; there
 * a trade whose bucket or whose flows leave 0 .. n_fix / 0 .. n_flt makes its chunk read nothing and its cell's sums NaN.
 *
 * adr_credit_subbook_ladders: host arrays, builds the cells and the plan itself, blocks (one allocation).  _dev: device
 * arrays - C, cell_plan_dev = adr_scenario_subbook_plan(n, C, cell_off), desk_cell_off_dev[B + 1] (sub-book b owns the
 * cells desk_cell_off[b] .. desk_cell_off[b + 1]) and cell_bucket_dev[C] -, enqueues on `stream` (NULL: the ctx's own)
 * without allocation, synchronisation or atomics to global memory.  adr_credit_subbook_ladders_work is its scratch in
 * doubles, (ceil(n / 64) + 2 C + B) records, and leaves the rows of chunk records in *chunks when that is not NULL.
 * _host: the CPU twin on the curve's arrays and a TradeBatch's: the same node, sum and projection code, chunks and orders.
 */
int64_t adr_credit_subbook_ladders_work(const adr_curve* curve, int64_t n, int64_t B, int64_t C, uint32_t req_mask, int64_t* chunks);
int adr_credit_subbook_ladders(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, const double* z, const int32_t* bucket,
                               int64_t n_fix, const double* fix_tau, int64_t n_flt, const double* flt_tau, int G, int64_t B,
                               const int64_t* sub_off, uint32_t req_mask, double* out);
int adr_credit_subbook_ladders_dev(adr_ctx* ctx, const adr_curve* curve, const adr_trades* trades, const double* z_dev,
                                   const int32_t* bucket_dev, int64_t n_fix, const double* fix_tau_dev, int64_t n_flt,
                                   const double* flt_tau_dev, int G, int64_t B, int64_t C, const int64_t* cell_plan_dev,
                                   const int64_t* desk_cell_off_dev, const int32_t* cell_bucket_dev, uint32_t req_mask,
                                   double* out_dev, double* work_dev, void* stream);
int adr_credit_subbook_ladders_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac,
                                    const double* hess, int64_t n, const int64_t* fix_off, const int64_t* flt_off,
                                    const double* fix_tp, const double* fix_pay, const double* flt_tp, const double* flt_ts,
                                    const double* flt_te, const double* flt_alpha, const double* flt_weight, const double* notional,
                                    const double* spread, const double* fix_sign, const double* flt_sign, const double* z,
                                    const int32_t* bucket, const double* fix_tau, const double* flt_tau, int G, int64_t B,
                                    const int64_t* sub_off, uint32_t req_mask, double* out);

/*
 * Inflation sub-book Greeks: per-desk PV, discount ladders, breakeven ladders and the discount x breakeven cross gamma of
 * one YoY book from ONE launch chain (csrc/yoy_subbook_ladder.hip), instead of one adr_yoy_risk plus one adr_price per desk.
 *
 * The discount curve is an uploaded adr_curve (adr_subbook_ladders' knot tables; the _host twin takes its raw arrays as
 * adr_subbook_ladders_host does).  The inflation curve is (infl_method, P_i, T[P_i], b[P_i]) as adr_yoy_risk takes it and
 * the book (n swaps; fix_off[n + 1], fix_tp, fix_pay [n_fix]; cpn_off[n + 1], cpn [ADR_YOY_FIELDS][m]) as
 * adr_yoy_scenario_subbook_pv takes it.  Sub-book b holds the swaps sub_off[b] .. sub_off[b + 1].
 *
 * out[B][1 + Q + Q*Q], Q = P_d + P_i (the discount pillars first, then the inflation curve's), one augmented row per
 * sub-book in adr_price's `agg` layout, out[b] = [pv, delta'[Q], gamma'[Q][Q]]:
 *
 *   pv                                      fixed legs plus YoY coupons (tp > 0)
 *   delta'[p < P_d], gamma'[p][q]           the discount ladders of the desk's cash flows, per bp and bp^2: the fixed flows and
 *                                           each coupon's projected amount as a fixed flow at tp (adr_subbook_ladders' nodes)
 *   delta'[P_d + k], gamma'[P_d+k][P_d+l]   breakeven delta per bp and gamma per bp^2, adr_yoy_risk's closed form: per coupon,
 *                                           g = scale E (1 + y), g u_k and g (u_k u_l + [k == l] v_k) over its live slots
 *   gamma'[p][P_d + k] = gamma'[P_d + k][p] d2PV / dquote_p db_k per bp^2, 1e-8 sum_a M[a][k] LJ[a][p] with M the knot-space
 *                                           mixed sum: ONE value stored twice.  adr_price and adr_yoy_risk do not have it.
 *
 * so adr_ladder_pnl* with P := Q and shock rows [x_bp[P_d], (b - b0) * 1e4 [P_i]] gives the joint second-order expansion.
 * E is the discount factor at tp as the knot tables give it, with NO division by D(0); adr_yoy_risk divides by D(0), and the
 * two agree where D(0) == 1.0, which holds on every curve the engine builds.  pv always, delta' with ADR_REQ_DELTA or
 * ADR_REQ_GAMMA, gamma' with ADR_REQ_GAMMA; blocks not requested are +0.0.  The entries write and do not add.
 *
 * A chunk (at most ADR_SCENARIO_CHUNK swaps of ONE sub-book) gives the record [pv, w[Kc], D[Kc], O[Kc], di[P_i],
 * gi[P_i][P_i], M[P_i][Kc]] (without GAMMA [pv, w[Kc], di[P_i]]); a sub-book's records are added in the plan's order by
 * adr_subbook_ladders' rule and the row is projected from the sums.  Contract: a sub-book's row has exactly the bits of the
 * same entry called with B = 1 on that sub-book's swaps alone - on the host twin and on the device -, does not depend on B
 * or on the other sub-books, and repeats bit for bit from run to run; an empty sub-book's row is +0.0 throughout; gamma' is
 * symmetric bit for bit in its cross rows and columns.  The device part rests on the same observed ordering of the LDS adds
 * (ds_add_f64) as adr_subbook_ladders.  On the host twin the discount block has the bits of adr_subbook_ladders_host on the
 * batch that holds, per swap, its fixed flows followed by its coupons' amounts as fixed flows.
 *
 * Refused: an inflation scheme other than LINEAR_ZERO_RATES / FLAT_FWD_RATES, P_i outside 1 .. ADR_YOY_MAX_PILLARS, a curve
 * pair whose tables for one wave (8 (3 Kc + P_i + P_i^2 + Kc P_i) bytes with GAMMA, 8 (Kc + P_i) without) do not fit the
 * LDS (all ADR_ERR_UNSUPPORTED); GAMMA on a curve uploaded without hess, null arrays, B < 1, n < 1 (ADR_ERR_INVALID); by the
 * blocking entry and the host twin also what they can read: pillars, rates, offsets and flows as adr_yoy_scenario_pv checks
 * them, sub_off as adr_scenario_subbook_plan does.  _dev checks scalars only; there a swap whose leg offsets leave
 * 0 .. n_fix / 0 .. m makes its chunk read nothing and its sub-book's row NaN, and no other row.
 *
 * adr_yoy_subbook_ladders: host arrays, builds the plan itself, blocks (one allocation).  _dev: device arrays and
 * plan_dev = adr_scenario_subbook_plan(n, B, sub_off), enqueues on `stream` (NULL: the ctx's own) without allocation,
 * synchronisation or atomics to global memory.  adr_yoy_subbook_ladders_work is its scratch in doubles,
 * (ceil(n / 64) + 2 B) records, and leaves the rows of chunk records in *chunks when that is not NULL.
 */
int64_t adr_yoy_subbook_ladders_work(const adr_curve* curve, int P_i, int64_t n, int64_t B, uint32_t req_mask, int64_t* chunks);
int adr_yoy_subbook_ladders(adr_ctx* ctx, const adr_curve* curve, int infl_method, int P_i, const double* T, const double* b, int64_t n,
                            int64_t n_fix, const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                            const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, uint32_t req_mask,
                            double* out);
int adr_yoy_subbook_ladders_dev(adr_ctx* ctx, const adr_curve* curve, int infl_method, int P_i, const double* T_dev, const double* b_dev,
                                int64_t n, int64_t n_fix, const int64_t* fix_off_dev, const double* fix_tp_dev,
                                const double* fix_pay_dev, int64_t m, const int64_t* cpn_off_dev, const double* cpn_dev, int64_t B,
                                const int64_t* plan_dev, uint32_t req_mask, double* out_dev, double* work_dev, void* stream);
int adr_yoy_subbook_ladders_host(int interp_method, int K, int P, const double* times, const double* dfs, const double* jac,
                                 const double* hess, int infl_method, int P_i, const double* T, const double* b, int64_t n,
                                 int64_t n_fix, const int64_t* fix_off, const double* fix_tp, const double* fix_pay, int64_t m,
                                 const int64_t* cpn_off, const double* cpn, int64_t B, const int64_t* sub_off, uint32_t req_mask,
                                 double* out);

/* Wait for everything enqueued on the ctx's own stream. */
int adr_sync(adr_ctx* ctx);

/*
 * Sum the aggregate ladder over the ranks of an RCCL communicator (one rank per
 * GPU): in-place ncclAllReduce(sum, double) of `count` doubles at agg_dev on
 * `stream`.  `rccl_comm` is an ncclComm_t.  This is the only exchange step of
 * the multi-GPU path; per-trade results never leave their GPU.
 */
int adr_allreduce_agg(adr_ctx* ctx, void* rccl_comm, double* agg_dev, int count, void* stream);

/*
 * The communicator for adr_allreduce_agg, for hosts that have no RCCL binding of their own (one rank per GPU / process):
 * rank 0 draws a unique id (adr_rccl_unique_id: ADR_RCCL_ID_BYTES bytes, = ncclGetUniqueId), hands it to the other ranks
 * by whatever channel the host has (a file, a socket, torch.distributed's store), and every rank calls adr_rccl_comm_init
 * with the same id (= ncclCommInitRank on the ctx's GPU; blocks until all n_ranks have called it).  The handle is an
 * ncclComm_t; free it with adr_rccl_comm_destroy before the ctx.
 */
#define ADR_RCCL_ID_BYTES 128
int adr_rccl_unique_id(void* id_out);
int adr_rccl_comm_init(adr_ctx* ctx, const void* id, int n_ranks, int rank, void** comm_out);
void adr_rccl_comm_destroy(void* rccl_comm);

#ifdef __cplusplus
}
#endif
#endif /* ADRATES_H */
