// Schedule groups of a batch (schedule_groups.hpp): hash the key, confirm by comparison, test the fixed leg's shape; and the
// host image of the device tables of the groups in use.
#include "schedule_groups.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

#include "host_pool.hpp"

namespace adr {

namespace {

inline uint64_t bits_of(double x) {
    uint64_t u;
    std::memcpy(&u, &x, sizeof u);
    return u;
}

// one multiply per value and an accumulator per array: the five chains of a trade run side by side
inline uint64_t step(uint64_t h, double v) { return (h ^ bits_of(v)) * 0x9e3779b97f4a7c15ull; }
inline uint64_t fold(uint64_t h) {
    h ^= h >> 32;
    h *= 0xff51afd7ed558ccdull;
    return h ^ (h >> 29);
}

uint64_t key_hash(const CsrHost& c, int64_t t) {
    const int64_t f0 = c.fix_off[t], f1 = c.fix_off[t + 1], l0 = c.flt_off[t], l1 = c.flt_off[t + 1];
    uint64_t h0 = static_cast<uint64_t>(f1 - f0) * 64 + static_cast<uint64_t>(l1 - l0) + 1, h1 = 1, h2 = 2, h3 = 3, h4 = 4;
    h0 = step(h0, c.spread[t]);
    for (int64_t j = f0; j < f1; ++j) h0 = step(h0, c.fix_tp[j]);
    for (int64_t j = l0; j < l1; ++j) {
        h1 = step(h1, c.flt_tp[j]);
        h2 = step(h2, c.flt_ts[j]);
        h3 = step(h3, c.flt_te[j]);
        h4 = step(h4, c.flt_alpha[j]);
    }
    return fold(fold(fold(fold(fold(h0) + h1) + h2) + h3) + h4);
}

bool same_key(const CsrHost& c, int64_t a, int64_t b) {
    const int64_t fa = c.fix_off[a], fb = c.fix_off[b], la = c.flt_off[a], lb = c.flt_off[b];
    const int64_t mf = c.fix_off[a + 1] - fa, ml = c.flt_off[a + 1] - la;
    if (mf != c.fix_off[b + 1] - fb || ml != c.flt_off[b + 1] - lb) return false;
    if (bits_of(c.spread[a]) != bits_of(c.spread[b])) return false;
    const size_t nf = static_cast<size_t>(mf) * sizeof(double), nl = static_cast<size_t>(ml) * sizeof(double);
    return (nf == 0 || std::memcmp(c.fix_tp + fa, c.fix_tp + fb, nf) == 0) &&
           (nl == 0 || (std::memcmp(c.flt_tp + la, c.flt_tp + lb, nl) == 0 && std::memcmp(c.flt_ts + la, c.flt_ts + lb, nl) == 0 &&
                        std::memcmp(c.flt_te + la, c.flt_te + lb, nl) == 0 && std::memcmp(c.flt_alpha + la, c.flt_alpha + lb, nl) == 0));
}

struct Found {                        // one group of a partition
    std::vector<int32_t> members;     // ascending
    std::vector<double> shape;        // x^ [n_fix]
};

// The trades of one key (ascending): those whose fixed leg has the key's shape form the group, the others stay ungrouped.
void close_class(const CsrHost& c, const std::vector<int32_t>& cls, std::vector<Found>& found) {
    if (cls.size() < 2) return;
    const int64_t mf = c.fix_off[cls[0] + 1] - c.fix_off[cls[0]];
    Found f;
    f.shape.assign(static_cast<size_t>(mf), 0.0);
    if (mf > 0) {
        // the shape: of the first trade that has a last payment
        for (int32_t t : cls) {
            const double* pay = c.fix_pay + c.fix_off[t];
            if (pay[mf - 1] == 0.0) continue;
            for (int64_t j = 0; j < mf; ++j) f.shape[static_cast<size_t>(j)] = pay[j] / pay[mf - 1];
            break;
        }
    }
    for (int32_t t : cls) {
        bool ok = true;
        if (mf > 0) {
            const double* pay = c.fix_pay + c.fix_off[t];
            const double last = pay[mf - 1];
            if (last == 0.0) {
                for (int64_t j = 0; j < mf; ++j) ok &= pay[j] == 0.0;        // a whole leg of zeros: cX = 0
            } else {
                const double a = std::fabs(last);
                const double tol = kScheduleShapeUlps * (std::nextafter(a, INFINITY) - a);
                for (int64_t j = 0; j < mf; ++j) ok &= std::fabs(pay[j] - last * f.shape[static_cast<size_t>(j)]) <= tol;
            }
        }
        if (ok) f.members.push_back(t);
    }
    if (f.members.size() >= 2) found.push_back(std::move(f));
}

}  // namespace

void build_schedule_groups(const CsrHost& c, const int32_t* eligible, int64_t n_eligible, ScheduleGroups& out) {
    out = ScheduleGroups();
    out.group_of.assign(static_cast<size_t>(c.n), -1);
    out.cF.assign(static_cast<size_t>(c.n), 0.0);
    out.cX.assign(static_cast<size_t>(c.n), 0.0);
    out.fix_off.assign(1, 0);
    out.flt_off.assign(1, 0);
    if (n_eligible < 2) return;

    // 1. hashes, a range of the list per thread
    const int n_threads = pool_threads(n_eligible, 4096);
    std::vector<std::pair<uint64_t, int32_t>> keyed(static_cast<size_t>(n_eligible));
    parallel_ranges(n_eligible, n_threads, [&](int, int64_t i0, int64_t i1) {
        for (int64_t i = i0; i < i1; ++i) keyed[static_cast<size_t>(i)] = {key_hash(c, eligible[i]), eligible[i]};
    });
    // 2. cut by hash into one partition per thread (equal keys share a partition)
    const uint64_t parts = static_cast<uint64_t>(n_threads);
    auto part_of = [&](uint64_t h) { return static_cast<size_t>((h >> 32) * parts >> 32); };
    std::vector<size_t> start(parts + 1, 0);
    for (const auto& k : keyed) ++start[part_of(k.first) + 1];
    for (size_t p = 0; p < parts; ++p) start[p + 1] += start[p];
    std::vector<std::pair<uint64_t, int32_t>> cut(keyed.size());
    {
        std::vector<size_t> at(start.begin(), start.end() - 1);
        for (const auto& k : keyed) cut[at[part_of(k.first)]++] = k;
    }
    // 3. per partition: sort by (hash, trade), split the runs of one hash into keys by comparison, test the shapes
    std::vector<std::vector<Found>> found(parts);
    parallel_ranges(static_cast<int64_t>(parts), n_threads, [&](int, int64_t p0, int64_t p1) {
        for (int64_t p = p0; p < p1; ++p) {
            auto first = cut.begin() + static_cast<std::ptrdiff_t>(start[static_cast<size_t>(p)]);
            auto last = cut.begin() + static_cast<std::ptrdiff_t>(start[static_cast<size_t>(p) + 1]);
            std::sort(first, last);
            std::vector<std::vector<int32_t>> classes;
            for (auto run = first; run != last;) {
                auto end = run;
                while (end != last && end->first == run->first) ++end;
                classes.clear();
                for (auto it = run; it != end; ++it) {
                    size_t k = 0;
                    while (k < classes.size() && !same_key(c, classes[k][0], it->second)) ++k;
                    if (k == classes.size()) classes.emplace_back();
                    classes[k].push_back(it->second);
                }
                for (const auto& cls : classes) close_class(c, cls, found[static_cast<size_t>(p)]);
                run = end;
            }
        }
    });
    // 4. number the groups by their lowest trade, write the members' coefficients and the basis trades
    std::vector<const Found*> order;
    for (const auto& part : found)
        for (const Found& f : part) order.push_back(&f);
    std::sort(order.begin(), order.end(), [](const Found* a, const Found* b) { return a->members[0] < b->members[0]; });
    out.n_groups = static_cast<int64_t>(order.size());
    out.size.reserve(order.size());
    for (const Found* f : order) {
        out.size.push_back(static_cast<int32_t>(f->members.size()));
        out.n_grouped += static_cast<int64_t>(f->members.size());
    }
    // (the members' entries: a range of the groups, then a range of the trades per thread - the second pass streams)
    parallel_ranges(out.n_groups, pool_threads(out.n_grouped, 4096), [&](int, int64_t g0, int64_t g1) {
        for (int64_t g = g0; g < g1; ++g)
            for (int32_t t : order[static_cast<size_t>(g)]->members) out.group_of[static_cast<size_t>(t)] = static_cast<int32_t>(g);
    });
    parallel_ranges(c.n, pool_threads(c.n, 4096), [&](int, int64_t t0, int64_t t1) {
        for (int64_t t = t0; t < t1; ++t) {
            if (out.group_of[static_cast<size_t>(t)] < 0) continue;
            const int64_t mf = c.fix_off[t + 1] - c.fix_off[t];
            out.cF[static_cast<size_t>(t)] = c.flt_sign[t] * c.notional[t];
            out.cX[static_cast<size_t>(t)] = mf > 0 ? c.fix_sign[t] * c.fix_pay[c.fix_off[t + 1] - 1] : 0.0;
        }
    });
    for (size_t g = 0; g < order.size(); ++g) {
        const Found& f = *order[g];
        const int64_t rep = f.members[0];
        const int64_t f0 = c.fix_off[rep], mf = c.fix_off[rep + 1] - f0, l0 = c.flt_off[rep], ml = c.flt_off[rep + 1] - l0;
        // 2g: the float leg
        out.flt_tp.insert(out.flt_tp.end(), c.flt_tp + l0, c.flt_tp + l0 + ml);
        out.flt_ts.insert(out.flt_ts.end(), c.flt_ts + l0, c.flt_ts + l0 + ml);
        out.flt_te.insert(out.flt_te.end(), c.flt_te + l0, c.flt_te + l0 + ml);
        out.flt_alpha.insert(out.flt_alpha.end(), c.flt_alpha + l0, c.flt_alpha + l0 + ml);
        out.flt_off.push_back(static_cast<int64_t>(out.flt_tp.size()));
        out.fix_off.push_back(static_cast<int64_t>(out.fix_tp.size()));
        out.notional.push_back(1.0);
        out.spread.push_back(c.spread[rep]);
        // 2g + 1: the fixed leg
        out.fix_tp.insert(out.fix_tp.end(), c.fix_tp + f0, c.fix_tp + f0 + mf);
        out.fix_pay.insert(out.fix_pay.end(), f.shape.begin(), f.shape.end());
        out.flt_off.push_back(static_cast<int64_t>(out.flt_tp.size()));
        out.fix_off.push_back(static_cast<int64_t>(out.fix_tp.size()));
        out.notional.push_back(0.0);
        out.spread.push_back(0.0);
    }
    out.sign.assign(2 * order.size(), 1.0);
}

GroupTables build_group_tables(const ScheduleGroups& F, const int32_t* rows_order, int64_t n_rows, int min_group,
                               int64_t min_grouped, int segment) {
    GroupTables T;
    // the groups in use, renumbered in order
    std::vector<int32_t> new_id(static_cast<size_t>(F.n_groups), -1);
    std::vector<int64_t> first;              // first record of every group in use, then the total
    for (int64_t g = 0; g < F.n_groups; ++g)
        if (F.size[static_cast<size_t>(g)] >= min_group) {
            new_id[static_cast<size_t>(g)] = static_cast<int32_t>(T.used_groups++);
            first.push_back(T.used_trades);
            T.used_trades += F.size[static_cast<size_t>(g)];
        }
    first.push_back(T.used_trades);
    if (T.used_groups == 0 || T.used_trades < min_grouped) return GroupTables();
    const size_t ng = static_cast<size_t>(T.used_groups);

    // records sorted by group, in trade order inside a group; the coefficient sums in trade order
    T.rec.resize(static_cast<size_t>(T.used_trades));
    T.sum_f.assign(ng, 0.0);
    T.sum_x.assign(ng, 0.0);
    {
        std::vector<int64_t> at(first.begin(), first.end() - 1);
        const int64_t n = static_cast<int64_t>(F.group_of.size());
        for (int64_t t = 0; t < n; ++t) {
            const int32_t old = F.group_of[static_cast<size_t>(t)];
            const int32_t g = old >= 0 ? new_id[static_cast<size_t>(old)] : -1;
            if (g < 0) continue;
            T.rec[static_cast<size_t>(at[static_cast<size_t>(g)]++)] =
                GroupRecord{static_cast<int32_t>(t), g, F.cF[static_cast<size_t>(t)], F.cX[static_cast<size_t>(t)], 0};
            T.sum_f[static_cast<size_t>(g)] += F.cF[static_cast<size_t>(t)];
            T.sum_x[static_cast<size_t>(g)] += F.cX[static_cast<size_t>(t)];
        }
    }
    // segments: no wave straddles two groups
    for (size_t g = 0; g < ng; ++g)
        for (int64_t at = first[g]; at < first[g + 1]; at += segment)
            T.seg.push_back(GroupSegment{static_cast<int32_t>(g), static_cast<int32_t>(at),
                                         static_cast<int32_t>(std::min<int64_t>(segment, first[g + 1] - at)), 0});
    // the plain rows outside the groups in use, in the table's order
    for (int64_t i = 0; i < n_rows; ++i) {
        const int32_t old = F.group_of[static_cast<size_t>(rows_order[i])];
        if (old < 0 || new_id[static_cast<size_t>(old)] < 0) T.rest.push_back(rows_order[i]);
    }
    // the basis trades of the groups in use: a small CSR batch of their own
    T.fix_off.assign(1, 0);
    T.flt_off.assign(1, 0);
    for (int64_t g = 0; g < F.n_groups; ++g) {
        if (new_id[static_cast<size_t>(g)] < 0) continue;
        for (int64_t k = 2 * g; k < 2 * g + 2; ++k) {
            const size_t f0 = static_cast<size_t>(F.fix_off[static_cast<size_t>(k)]), f1 = static_cast<size_t>(F.fix_off[static_cast<size_t>(k) + 1]);
            const size_t l0 = static_cast<size_t>(F.flt_off[static_cast<size_t>(k)]), l1 = static_cast<size_t>(F.flt_off[static_cast<size_t>(k) + 1]);
            T.fix_tp.insert(T.fix_tp.end(), F.fix_tp.begin() + f0, F.fix_tp.begin() + f1);
            T.fix_pay.insert(T.fix_pay.end(), F.fix_pay.begin() + f0, F.fix_pay.begin() + f1);
            T.flt_tp.insert(T.flt_tp.end(), F.flt_tp.begin() + l0, F.flt_tp.begin() + l1);
            T.flt_ts.insert(T.flt_ts.end(), F.flt_ts.begin() + l0, F.flt_ts.begin() + l1);
            T.flt_te.insert(T.flt_te.end(), F.flt_te.begin() + l0, F.flt_te.begin() + l1);
            T.flt_alpha.insert(T.flt_alpha.end(), F.flt_alpha.begin() + l0, F.flt_alpha.begin() + l1);
            T.fix_off.push_back(static_cast<int64_t>(T.fix_tp.size()));
            T.flt_off.push_back(static_cast<int64_t>(T.flt_tp.size()));
            T.notional.push_back(F.notional[static_cast<size_t>(k)]);
            T.spread.push_back(F.spread[static_cast<size_t>(k)]);
        }
    }
    T.sign.assign(2 * ng, 1.0);
    T.rows.resize(2 * ng);
    for (size_t k = 0; k < 2 * ng; ++k) T.rows[k] = static_cast<int32_t>(k);
    return T;
}

}  // namespace adr
