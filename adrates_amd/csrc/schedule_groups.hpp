// Schedule groups: the trades of a batch that share their whole remaining schedule, found at upload (host only, no HIP).
//
// A trade's ladder [PV, delta, gamma] is linear in its cash amounts; everything non-linear (lookups, exponentials, Jacobian
// rows, rank-one updates, convexity rows) depends on its node times only.  Two trades with the same times and spread whose
// fixed payments are proportional therefore differ by two coefficients:
//   ladder(t) = cF(t) * BF[g] + cX(t) * BX[g],   cF = flt_sign * notional,   cX = fix_sign * fix_pay[last]
// with BF the ladder of the group's float leg per unit notional (at the group's spread) and BX that of its fixed leg per unit
// of the last payment (x^_j = fix_pay[j] / fix_pay[last] of the group's first trade that has a last payment).  The pricing
// call prices the two basis trades of every group once and forms the members' ladders in a store pass (kernels_combine.hip).
// DESIGN.md section 22.
#pragma once
#include <cstdint>
#include <vector>

namespace adr {

constexpr int kScheduleShapeUlps = 16;      // a member's fixed payments match last * x^ to this many ulps of the last payment

// The caller's CSR batch on the host (the arrays of adr_trades_upload).
struct CsrHost {
    int64_t n;
    const int64_t *fix_off, *flt_off;
    const double *fix_tp, *fix_pay, *flt_tp, *flt_ts, *flt_te, *flt_alpha;
    const double *notional, *spread, *fix_sign, *flt_sign;
};

struct ScheduleGroups {
    int64_t n_groups = 0;            // groups of at least two trades, numbered by their lowest trade index
    int64_t n_grouped = 0;           // trades in them
    std::vector<int32_t> group_of;   // [n] the trade's group, -1: ungrouped
    std::vector<int32_t> size;       // [n_groups]
    std::vector<double> cF, cX;      // [n] the member's coefficients (0 for ungrouped trades)
    // The basis trades as a CSR batch of 2 n_groups pseudo-trades: 2g the float leg of group g (notional 1, the group's
    // spread, no fixed flows), 2g + 1 its fixed leg x^ (no float coupons, notional 0); every sign +1.
    std::vector<int64_t> fix_off, flt_off;
    std::vector<double> fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, notional, spread, sign;
};

// eligible[0 .. n_eligible): the trades of the plain one-row table (no payment lag, no weights, at most 32 coupons per leg).
// Nothing in the decision depends on notionals, coupon levels or signs: the key is the coupon counts and the bit patterns of
// the times, accrual fractions and spread, the shape test is relative to the trade's own last payment.
void build_schedule_groups(const CsrHost& csr, const int32_t* eligible, int64_t n_eligible, ScheduleGroups& out);

// What the store pass reads (kernels.hpp, CombineDev; kernels_combine.hip): the members' ladders from their group's two basis
// ladders.
struct GroupRecord {              // 32 bytes, read with scalar loads; sorted by group, trade order inside a group
    int32_t trade, group;
    double cF, cX;                // out[trade] = cF * BF[group] + cX * BX[group]
    int64_t pad;
};
static_assert(sizeof(GroupRecord) == 32, "GroupRecord is read as 32-byte records");
struct GroupSegment {             // the records one wave writes: all of one group
    int32_t group, first, count, pad;
};

// The host image of the device tables of the groups IN USE (renumbered in order): what the batch uploads for the grouped
// route.  used_groups == 0: the route is not taken and every vector is empty.
struct GroupTables {
    int64_t used_groups = 0, used_trades = 0;
    std::vector<GroupRecord> rec;        // [used_trades] sorted by group, in trade order inside a group
    std::vector<GroupSegment> seg;       // they tile `rec`; no segment straddles two groups or exceeds the length asked for
    std::vector<double> sum_f, sum_x;    // [used_groups] the members' coefficient sums, taken in TRADE order (the grouped
                                         // aggregate must not depend on the segment length)
    std::vector<int32_t> rest;           // the trades of the plain row table outside the groups in use, in the table's order
    // the basis trades of the groups in use: the CSR batch of ScheduleGroups cut down to them, every sign +1, and its row list
    std::vector<int64_t> fix_off, flt_off;
    std::vector<double> fix_tp, fix_pay, flt_tp, flt_ts, flt_te, flt_alpha, notional, spread, sign;
    std::vector<int32_t> rows;           // [2 used_groups] the identity
};

// A group is used from `min_group` trades on; the route is taken when the groups in use hold at least `min_grouped` trades
// (0: whatever they hold).  rows_order[0 .. n_rows): the plain row table's trades in table order; `segment`: records per
// segment (>= 1).  Host only.
GroupTables build_group_tables(const ScheduleGroups& found, const int32_t* rows_order, int64_t n_rows, int min_group,
                               int64_t min_grouped, int segment);

}  // namespace adr
