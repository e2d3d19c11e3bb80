"""adr_bond_measures_host and adr_frn_measures_host held to the plain 60-digit reference of tests/_measures_reference.py, every
output of every instrument on its counted bound |got - value| <= k 2^-53 gross; the solved outputs (z, the yield, the DM) by
their exact residual at the returned root; the status by the exact sign change over the bracket.  The books and curves are
those of tests/_measures_cases.py - every edge bond x curve x scheme and every edge FRN x curve pair x scheme in both quote modes,
the raw books on node times - and its solver edges: quotes at the bracket ends on the 600-flow instruments, a status-1 and a
status-2 row past the register windows (129 flows, 385 coupons), matured bonds, an FRN whose cap equals its floor and one with a
negative floored rate.  No GPU.

Measured on the host twins (the worst |error| / allowance over all cases; nothing beyond <= 1.0 is asserted):
  bonds  z 0.127, dirty 0.180, clean 0.170, ytm 0.419, duration 0.104, convexity 0.0834, dv01 0.0858;  k_P 12 .. 2443 (dirty
         14 .. 2445, dv01 13 .. 2469), k of the yield passes 7 .. 75 (duration 9 .. 77, convexity 10 .. 78);  residuals up to
         4.35 units of gross for z (stop term up to 126) and, midpoint case apart, 63 for the yield; 252 in the midpoint
         case of tests/_measures_reference.py (the 600-flow bond at z = -0.1; stop term 412)
  FRNs   dm 0.0883, dirty 0.096, clean 0.0456, pv 0.106, mod_duration 0.0697, dv01 0.0454;  k_P 17 .. 5182 (mod_duration
         21 .. 5196);  the DM's residual up to 1.77 units of gross, the stop term up to 0.576
  cond's share of k_P: 0.03 .. 0.98 (bonds), 0.11 .. 0.99 (FRNs): beyond the last node it is nearly all of k.
`test_bound_rejects_subtly_wrong_variants` shows that the same bound fails six plain float64 variants that are each wrong
in one small way."""
import math

import numpy as np
import pytest

from adrates_amd import _native

from . import _measures_cases as C
from . import _measures_reference as R
from .test_measures_edges_host import CURVE_CASES, PAIR_CASES, ids

TOTAL = {}                          # what: the merged `Report` of the cases run so far, printed by the last test of a module


def hold(rep, what, into, want_status=None):
    """Prints ``rep``, asserts the statuses and the bound, merges it into ``TOTAL[into]``."""
    print(rep.line(what))
    assert not rep.status_bad, f"{what}: (row, status, the reference's) {rep.status_bad}"
    if want_status is not None:
        assert rep.status_want == list(want_status), (what, rep.status_want)
    bad = {o: r for o, r in rep.ratio.items() if not r <= 1.0}
    assert not bad, f"{what}: beyond the bound: {bad}"
    if into in TOTAL:
        TOTAL[into].merge(rep)
    else:
        TOTAL[into] = rep


def bond_books(scheme, curve_name):
    """``[(what, (method, node_t, node_df, book), quote_is_z, the statuses the case is built for or None)]``."""
    curve, prices, _ = C.bond_refs(scheme, curve_name)
    bonds = [b for _, b, _ in C.edge_bonds()]
    return [("edge bonds at z", C.bond_arrays(bonds, curve, C.BOND_Z), True, None),
            ("edge bonds at clean prices", C.bond_arrays(bonds, curve, prices), False, None),
            ("solver edges at z", C.extra_bond_book(curve, True), True, None),
            ("solver edges at clean prices", C.extra_bond_book(curve, False), False, C.BOND_EXTRA_STATUS)]


def frn_books(scheme, disc_name, index_name):
    """``[(what, (disc, index, book), quote_is_dm, statuses or None)]``."""
    disc, index, prices, _ = C.frn_refs(scheme, disc_name, index_name)
    frns = [f for _, f, _ in C.edge_frns()]
    return [("edge FRNs at DM", C.frn_arrays(frns, disc, index, C.FRN_DM), True, [0] * len(frns)),
            ("edge FRNs at clean prices", C.frn_arrays(frns, disc, index, prices), False, [0] * len(frns)),
            ("solver edges at DM", C.extra_frn_book(disc, index, True), True, [0] * 4),
            ("solver edges at clean prices", C.extra_frn_book(disc, index, False), False, C.FRN_EXTRA_STATUS)]


def node_books(scheme):
    """The raw books on node times: ``(bond args, FRN args)``."""
    t, d, book = C.bonds_on_nodes()
    (dt, dd), (it, idf), fbook = C.frns_on_nodes()
    return (scheme.value, t, d, book), ((scheme.value, dt, dd), (C.index_scheme(scheme).value, it, idf), fbook)


@pytest.mark.parametrize("case", CURVE_CASES, ids=ids)
def test_bond_host_within_the_bound(case):
    for what, args, is_z, status in bond_books(*case):
        got = _native.bond_measures_host(*args, is_z)
        hold(R.check_bonds(*args, is_z, got), f"host, {ids(case)}, {what}", "bond host", status)


@pytest.mark.parametrize("case", PAIR_CASES, ids=ids)
def test_frn_host_within_the_bound(case):
    for what, args, is_dm, status in frn_books(*case):
        got = _native.frn_measures_host(*args, is_dm)
        hold(R.check_frns(*args, is_dm, got), f"host, {ids(case)}, {what}", "frn host", status)


@pytest.mark.parametrize("scheme", C.SCHEMES, ids=lambda s: s.name)
def test_host_on_node_times_within_the_bound(scheme):
    bond, frn = node_books(scheme)
    hold(R.check_bonds(*bond, True, _native.bond_measures_host(*bond, True)), f"host, {scheme.name}, bonds on nodes",
         "bond host", [0, 0])
    hold(R.check_frns(*frn, True, _native.frn_measures_host(*frn, True)), f"host, {scheme.name}, FRNs on nodes", "frn host",
         [0, 3])


def test_reference_dates_take_every_branch():
    """D(t) of the reference where its value is known without it: the first node, before it, and - the two forward schemes
    being exact there - on a node; the first segment's and the extrapolation's closed forms on a 3-node table."""
    R.mp.dps = R.DPS
    x, d = np.array([0.0, 2.0, 5.0]), np.array([1.0, 0.9, 0.7])
    L = [math.log(v) for v in d]
    for method in (R.FLAT_FWD, R.LINEAR_FWD, R.LINEAR_ZERO):
        tab = R.Table(method, x, d)
        assert tab.date(0.0) == (1.0, 0, 0) and math.isnan(float(tab.date(-1e-9)[0]))
        assert float(tab.date(5.0)[0]) == pytest.approx(0.7, rel=1e-15)
    near = lambda got, want: abs(float(got[0]) - want) <= 2e-15 * want
    flat, lin, zero = (R.Table(m, x, d) for m in (R.FLAT_FWD, R.LINEAR_FWD, R.LINEAR_ZERO))
    assert near(flat.date(1.0), math.exp(0.5 * L[1])) and near(flat.date(8.0), 0.7 * (0.7 / 0.9) ** 1.0)
    assert near(zero.date(1.0), math.exp(L[1] / 2.0)) and near(zero.date(8.0), math.exp(L[2] / 5.0 * 8.0))
    assert near(lin.date(1.0), math.exp(math.log(0.9 + 1e-10) / (2.0 + 1e-10)))
    assert near(lin.date(2.0), math.exp(2.0 * math.log(0.9 + 1e-10) / (2.0 + 1e-10)))          # not d_1: the regulariser
    assert near(lin.date(8.0), 0.7 * (0.7 / 0.9) ** 1.0)
    f1, f2 = -L[1] / 2.0, -(L[2] - L[1]) / 3.0                                                  # the segments' forwards
    assert near(lin.date(3.5), 0.9 * math.exp(-0.5 * (f1 + f2) * 1.5))
    # the units grow with the conditioning: 50Y on a table that ends at 5Y
    assert zero.date(50.0)[1] > flat.date(50.0)[1] > flat.date(3.0)[1] >= 2


# ------------------------------------------------------------------------------------------------ subtly wrong variants
def _df64(t, x, d, method, keep_small=True):
    """node_df.hpp's rule in plain float64, for the variants below."""
    n = len(x)
    if t == x[0]:
        return d[0]
    i = next((k for k in range(n) if x[k] >= t), n)
    ln = math.log
    if method == R.LINEAR_ZERO:
        p, q, a, b = (1, 1, x[0], x[1]) if i == 1 else (i - 1, i, x[i - 1], x[i]) if i < n else (n - 1, n - 1, x[n - 2], x[n - 1])
        return math.exp(-(((b - t) * (-ln(d[p]) / x[p]) + (t - a) * (-ln(d[q]) / x[q])) / (b - a)) * t)
    if method == R.FLAT_FWD:
        p, q = (i - 1, i) if i < n else (n - 2, n - 1)
        return math.exp(-(((x[q] - t) * -ln(d[p]) + (t - x[p]) * -ln(d[q])) / (x[q] - x[p])))
    small = 1e-10 if keep_small else 0.0
    if i == 1:
        return math.exp(-(t * -ln(d[1] + small) / (x[1] + small)))
    fwd = -ln(d[i - 1] / d[i - 2]) / (x[i - 1] - x[i - 2])
    if i < n:
        fwd2 = -ln(d[i] / d[i - 1]) / (x[i] - x[i - 1])
        fwd = ((x[i] - t) * fwd + (t - x[i - 1]) * fwd2) / (x[i] - x[i - 1])
    return d[i - 1] * math.exp(-fwd * (t - x[i - 1]))


def _variant(method, x, d, book, keep_small=True, bump=1e-4, face_at_tauM=True, skip_unpaid=True, root_shift=0.0, drop=None):
    """adr_bond_measures' outputs for given z-spreads in plain float64 (exactly summed products, the yield by bisection to the
    last bit); each keyword away from its default is one fault.  ``drop``: (bond, flow) left out."""
    x, d = [float(v) for v in x], [float(v) for v in d]
    n = len(book["flow_off"]) - 1
    out = {o: np.empty(n) for o in R.BOND_OUTPUTS}
    out["status"] = np.zeros(n, dtype=np.int32)
    for b in range(n):
        flows = [i for i in range(book["flow_off"][b], book["flow_off"][b + 1]) if drop != (b, i - book["flow_off"][b])]
        Ds = _df64(float(book["bond_Ts"][b]), x, d, method, keep_small)
        f = lambda k, i: float(book[k][i])
        A = [(f("flow_cpn", i) + (max(f("flow_prin", i), 0.0) if skip_unpaid else f("flow_prin", i))) *
             (_df64(f("flow_T", i), x, d, method, keep_small) / Ds) for i in flows]
        tau = [f("flow_tau", i) for i in flows]
        P = lambda s: math.fsum(a * math.exp(-s * t) for a, t in zip(A, tau))
        face, tauM, acc, z = (float(book[k][b]) for k in ("bond_face", "bond_tauM", "bond_acc100", "bond_quote"))
        dirty = P(z) / face * 100.0
        clean = dirty - acc
        amounts, times = [f("flow_cpn", i) for i in flows], list(tau)
        if tauM > 0.0:
            amounts, times = amounts + [face], times + [tauM if face_at_tauM else tau[-1]]
        Y = lambda y, m=0: math.fsum(c * t ** m * math.exp(-y * t) for c, t in zip(amounts, times))
        y = C._bisect(lambda s: Y(s) - ((clean + acc) / 100.0) * face, -0.5, 0.5) + root_shift
        vals = {"z": z, "dirty": dirty, "clean": clean, "ytm": y, "duration": Y(y, 1) / Y(y), "convexity": Y(y, 2) / Y(y),
                "dv01": (P(z - bump) - P(z + bump)) / 2.0}
        for o, v in vals.items():
            out[o][b] = v
    return out


def _with_tiny_flow(book, b):
    """``book`` with one more flow behind bond b's last: a coupon of 1e-11 of the face on the last flow's date."""
    at = int(book["flow_off"][b + 1])
    out = dict(book)
    for k, v in (("flow_T", book["flow_T"][at - 1]), ("flow_tau", book["flow_tau"][at - 1]),
                 ("flow_cpn", 1e-11 * book["bond_face"][b]), ("flow_prin", 0.0)):
        out[k] = np.insert(book[k], at, v)
    out["flow_off"] = book["flow_off"].copy()
    out["flow_off"][b + 1:] += 1
    return out


def test_bound_rejects_subtly_wrong_variants():
    """The bound separates right from subtly wrong: a plain float64 evaluation of the documented formulas lies within it on
    every output, and each of six small faults breaks it on at least one."""
    scheme = C.InterpTypes.LINEAR_FWD_RATES
    curve = C.curves(scheme)["short_20y"]                           # monthly flows inside its first segment [0, 0.5]
    bonds = [b for _, b, _ in C.edge_bonds()][:5]                   # 1 .. 127 flows, two of them with a payment lag
    method, nt, nd, book = C.bond_arrays(bonds, curve, C.BOND_Z[:5])
    tiny_at = (1, int(book["flow_off"][2] - book["flow_off"][1]))   # behind the 15-flow bullet's last flow
    book = _with_tiny_flow(book, 1)
    assert np.any((book["flow_T"] > nt[0]) & (book["flow_T"] < nt[1]))
    assert np.any(book["flow_tau"][book["flow_off"][1:] - 1] != book["bond_tauM"])       # a payment lag: tau_M is not the last tau
    t, d, raw = C.bonds_on_nodes()
    assert np.any(raw["flow_prin"] < 0.0)
    worst = lambda args, **fault: R.check_bonds(*args, True, _variant(*args, **fault))
    right = worst((method, nt, nd, book))
    print(right.line("float64 restatement"))
    assert right.worst() <= 1.0 and not right.status_bad
    assert worst((method, t, d, raw)).worst() <= 1.0
    faults = {"the regulariser dropped": ((method, nt, nd, book), {"keep_small": False}),
              "a bump of 1.0001e-4": ((method, nt, nd, book), {"bump": 1.0001e-4}),
              "the face at the last flow's tau": ((method, nt, nd, book), {"face_at_tauM": False}),
              "a principal <= 0 paid": ((method, t, d, raw), {"skip_unpaid": False}),
              "a root moved by 1e-12": ((method, nt, nd, book), {"root_shift": 1e-12}),
              "a flow of 1e-11 of the face dropped": ((method, nt, nd, book), {"drop": tiny_at})}
    for name, (args, fault) in faults.items():
        rep = worst(args, **fault)
        broken = sorted(o for o, r in rep.ratio.items() if r > 1.0)
        print(f"{name}: breaks {broken}, worst ratio {rep.worst():.3g}")
        assert broken, name


def test_worst_ratios_of_the_host_twins():
    """Prints what the tests above found, all cases merged (run the module with -s to read it)."""
    for what in ("bond host", "frn host"):
        if what in TOTAL:
            print(TOTAL[what].line(what + ", all cases"))
            assert TOTAL[what].worst() <= 1.0
