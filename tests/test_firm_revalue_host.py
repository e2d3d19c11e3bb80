"""Full revaluation of a firm - rates, credit and inflation desks under joint shock rows - on the CPU twins
(market/position/monte_carlo_firm.py with ``host=True``), on the firm of tests/_firm_revalue_cases.py: the chain against
`combine_sub_book_rows` of the three ``*_on_curves_sub_books`` calls bit for bit, whatever the tiling; one line alone; the
ladders on the firm's columns; the tail figures; the third-order gap to delta-gamma; the refusals."""
import numpy as np
import pytest

from adrates_amd.market.position.engine import Engine
from adrates_amd.market.position.ladder_pnl import augmented_ladder_pnl
from adrates_amd.market.position.monte_carlo import (ShockedCurves, allocate_tail_select, monte_carlo_shocks, monte_carlo_var_es,
                                                     revalue_shocks_sub_books, tail_measures_select)
from adrates_amd.market.position.monte_carlo_firm import (FirmBook, embed_ladder_rows, firm_ladders, firm_scenario_bytes,
                                                          monte_carlo_explain_firm_var_es, monte_carlo_revalue_firm_var_es,
                                                          revalue_shocks_firm)
from adrates_amd.market.position.scenarios import combine_sub_book_rows, tail_count
from adrates_amd.utils.error import LibError

from . import _firm_revalue_cases as FC
from . import _tail_alloc_cases as TA


@pytest.fixture(scope="module")
def chain(native_lib):
    """The recipe, the three-line firm, its factor, the host's joint shock rows and the host chain's P&L, made once."""
    curves = FC.curves()
    firm = FC.firm(curves)
    factor = FC.factor(firm.n_columns)
    x = monte_carlo_shocks(factor, FC.CHAIN_S, FC.SEED, host=True)
    return dict(curves=curves, firm=firm, factor=factor, x=x, pnl=revalue_shocks_firm(firm, x, host=True))


def test_the_firm_and_its_columns(chain):
    firm, cols = chain["firm"], chain["firm"].columns
    assert firm.labels == FC.LABELS and chain["pnl"]["labels"] == FC.LABELS and chain["pnl"]["pnl"].shape == (5, FC.CHAIN_S)
    assert [line.kind for line in firm.lines] == ["rates", "credit", "inflation"]
    lines = [set(line.labels) for line in firm.lines]
    assert lines[0] & lines[1] & lines[2] == {"macro"} and {"credit", "frns"} <= lines[0] & lines[1] - lines[2]
    assert "swaps" in lines[0] - lines[1] - lines[2] and "linkers" in lines[2] - lines[0] - lines[1]
    assert (cols["curve"], cols["spread"], cols["breakeven"]) == (range(0, 32), range(32, 36), range(36, 56))
    assert sorted(cols["buckets"]) == sorted(FC.CL.EXPLAIN_BUCKETS) and cols["infl_tenors"][:3] == ["1Y", "2Y", "3Y"]
    assert len(cols["infl_tenors"]) == 20 and firm.n_columns == 56 and chain["pnl"]["columns"] == cols
    assert [list(line.add) for line in firm.lines] == [[0, 0, 0, 0], [1, 1, 1], [0, 1]]


def test_chain_has_the_bits_of_the_three_lines_combined(chain):
    parts = FC.line_rows(chain["curves"], chain["firm"], chain["x"])
    want = combine_sub_book_rows(parts)
    assert want["labels"] == FC.LABELS
    assert np.array_equal(FC.bits(chain["pnl"]["pnl"]), FC.bits(want["rows"][:, :-1] - want["rows"][:, -1:]))


def test_chain_does_not_depend_on_the_tiling(chain):
    firm = chain["firm"]
    per, rows = firm_scenario_bytes(firm), 8 * 5 * (FC.CHAIN_S + 1)
    for tile in FC.TILES:
        got = revalue_shocks_firm(firm, chain["x"], host=True, max_bytes=rows + tile * per)
        assert np.array_equal(FC.bits(got["pnl"]), FC.bits(chain["pnl"]["pnl"])), tile
    with pytest.raises(LibError, match="do not fit max_bytes"):
        revalue_shocks_firm(firm, chain["x"], host=True, max_bytes=rows + per - 1)


def test_zero_shock_row_is_exactly_zero(chain):
    x = chain["x"][:5].copy()
    x[2] = 0.0
    pnl = revalue_shocks_firm(chain["firm"], x, host=True)["pnl"]
    assert np.array_equal(FC.bits(pnl[:, 2]), FC.bits(np.zeros(5))) and np.all(pnl[:, [0, 1, 3, 4]] != 0.0)


@pytest.mark.parametrize("kind", ["rates", "credit", "inflation"])
def test_one_line_is_that_lines_own_call(chain, kind):
    """A firm of one line on the columns that line leaves: its own ``*_on_curves_sub_books`` call, and for rates
    `revalue_shocks_sub_books`."""
    curves = chain["curves"]
    firm = FC.firm(curves, kind)
    cols = chain["firm"].columns
    keep = list(cols["curve"]) + {"rates": [], "credit": list(cols["spread"]), "inflation": list(cols["breakeven"])}[kind]
    x = np.ascontiguousarray(chain["x"][:, keep])
    assert firm.n_columns == len(keep)
    got = revalue_shocks_firm(firm, x, host=True)
    (labels, rows), = FC.line_rows(curves, firm, x, kinds=(kind,))
    assert got["labels"] == labels and np.array_equal(FC.bits(got["pnl"]), FC.bits(rows[:, :-1] - rows[:, -1:]))
    if kind == "rates":             # `revalue_shocks_sub_books` wraps this very firm: the wrapper against what it wraps
        own = revalue_shocks_sub_books(curves, *FC.lines()["rates"], x, host=True)
        assert own["labels"] == labels and np.array_equal(FC.bits(got["pnl"]), FC.bits(own["pnl"]))


def test_ladders_on_the_firms_columns(chain):
    """`augmented_ladder_pnl` of `firm_ladders` is the sum, by label, of the three lines' delta-gamma P&L on their own
    columns, within the project's 1e-10 of the desk's sum of absolute terms; the embedding itself moves bits only."""
    firm, x = chain["firm"], chain["x"]
    engine = Engine(FC.model()[0])
    rows = firm_ladders(engine, firm, host=True)
    assert rows.shape == (5, 1 + 56 + 56 * 56)
    got = augmented_ladder_pnl(rows, x, host=True)
    parts = FC.line_delta_gamma(chain["curves"], firm, engine, x)
    want = FC.desk_sum(FC.LABELS, [(labs, o["pnl"]) for labs, o in parts])
    scale = FC.desk_sum(FC.LABELS, [(labs, np.abs(o["delta_pnl"]) + np.abs(o["gamma_pnl"])) for labs, o in parts])
    err = np.abs(got - want) / scale
    print("ladders on the firm's columns: worst error over the sum of absolute terms per desk", err.max(axis=1))
    assert np.all(scale > 0.0) and np.all(err <= 1e-10)
    small = np.arange(1.0, 1 + 1 + 2 + 4)[None, :]
    wide = embed_ladder_rows(small, [3, 1], 4)
    assert wide[0, 0] == 1.0 and np.array_equal(wide[0, 1:5], [0.0, 3.0, 0.0, 2.0])
    g = wide[0, 5:].reshape(4, 4)
    assert g[3, 3] == 4.0 and g[3, 1] == 5.0 and g[1, 3] == 6.0 and g[1, 1] == 7.0 and np.count_nonzero(g) == 4
    for cols in ([1, 1], [0, 4], [0]):
        with pytest.raises(LibError):
            embed_ladder_rows(small, cols, 4)


def test_var_es_and_allocation_are_the_tail_entries_of_the_rows(chain):
    firm, pnl = chain["firm"], chain["pnl"]["pnl"]
    per = firm_scenario_bytes(firm)
    for level in (0.99, 0.9):
        var, es = tail_measures_select(pnl, level, host=True)
        for max_bytes in (2 ** 31, 8 * 5 * (FC.CHAIN_S + 1) + 64 * per):
            got = monte_carlo_revalue_firm_var_es(firm, chain["factor"], FC.CHAIN_S, level=level, seed=FC.SEED, host=True, max_bytes=max_bytes)
            assert sorted(got) == ["es", "labels", "var"] and got["labels"] == FC.LABELS
            assert np.array_equal(FC.bits(got["var"]), FC.bits(var)) and np.array_equal(FC.bits(got["es"]), FC.bits(es)), level
        got = monte_carlo_revalue_firm_var_es(firm, chain["factor"], FC.CHAIN_S, level=level, seed=FC.SEED, host=True, allocate=True)
        whole = allocate_tail_select(pnl, level, host=True)
        assert np.array_equal(FC.bits(got["var"]), FC.bits(var)) and np.array_equal(FC.bits(got["es"]), FC.bits(es))
        assert got["firm_var"] == whole["var"] and got["firm_es"] == whole["es"]
        assert np.array_equal(FC.bits(got["comp_var"]), FC.bits(whole["comp_var"]))
        assert np.array_equal(FC.bits(got["comp_es"]), FC.bits(whole["comp_es"]))
        TA.check(dict(var=got["firm_var"], es=got["firm_es"], comp_var=got["comp_var"], comp_es=got["comp_es"]), pnl, -1,
                 tail_count(level, FC.CHAIN_S))


def test_explain_sets_the_two_routes_side_by_side(chain):
    firm, L = chain["firm"], chain["factor"]
    engine = Engine(FC.model()[0])
    got = monte_carlo_explain_firm_var_es(engine, firm, L, FC.CHAIN_S, level=0.9, seed=FC.SEED, host=True)
    full = monte_carlo_revalue_firm_var_es(firm, L, FC.CHAIN_S, level=0.9, seed=FC.SEED, host=True)
    dg = monte_carlo_var_es(None, None, L, FC.CHAIN_S, level=0.9, seed=FC.SEED, host=True, ladders=firm_ladders(engine, firm, host=True))
    assert got["labels"] == full["labels"] == FC.LABELS
    for key, ref in (("full_var", full["var"]), ("full_es", full["es"]), ("dg_var", dg["var"]), ("dg_es", dg["es"]),
                     ("gap_var", full["var"] - dg["var"]), ("gap_es", full["es"] - dg["es"])):
        assert np.array_equal(FC.bits(got[key]), FC.bits(ref)), key
    assert np.all(np.abs(got["gap_var"]) < 0.05 * np.abs(got["full_var"])), "the expansion describes these books at daily moves"


# ------------------------------------------------------------------------------------------ the reason for the feature
@pytest.mark.parametrize("kinds", [("credit",), ("inflation",), ()], ids=["credit", "inflation", "three_lines"])
def test_gap_to_delta_gamma_is_third_order(chain, kinds):
    """The same seed with the factor L and with L / 2: the rows are exact halves, and the worst |full - delta-gamma| over
    the scenarios, per desk, falls by about 8 - inside GAP_BAND for every desk, none dropped.  Observed on the host twins:
    credit only (frns, macro, credit) 7.935, 7.985, 7.985; inflation only (linkers, macro) 8.017, 8.078; three lines
    (macro, swaps, credit, frns, linkers) 7.990, 8.091, 8.134, 8.024, 7.985."""
    firm = chain["firm"] if not kinds else FC.firm(chain["curves"], *kinds)
    engine = Engine(FC.model()[0])
    L = FC.factor(firm.n_columns)
    x, half = (monte_carlo_shocks(s * L, FC.CHAIN_S, FC.SEED, host=True) for s in (1.0, 0.5))
    assert np.array_equal(FC.bits(half), FC.bits(0.5 * x))
    rows = firm_ladders(engine, firm, host=True)
    gap = [(revalue_shocks_firm(firm, s, host=True)["pnl"], augmented_ladder_pnl(rows, s, host=True)) for s in (x, half)]
    ratios = FC.gap_ratios(*gap[0], *gap[1])
    print("host: gap ratios per desk", firm.labels, np.round(ratios, 3))
    assert ratios.shape == (firm.n_desks,) and np.all((FC.GAP_BAND[0] < ratios) & (ratios < FC.GAP_BAND[1])), ratios


# ----------------------------------------------------------------------------------------------------------- refusals
def test_refusals(chain):
    from adrates_amd.trades.market_data import usd_model
    curves, firm, lines = chain["curves"], chain["firm"], FC.lines()
    with pytest.raises(LibError, match="at least one"):
        FirmBook(curves)
    with pytest.raises(LibError):
        FirmBook(FC.model()[0], rates=lines["rates"])
    usd = ShockedCurves(usd_model(FC.VD, FC.INTERP), "USD_OIS_SOFR")
    with pytest.raises(LibError, match="discounts on GBP_OIS_SONIA"):
        FirmBook(usd, inflation=lines["inflation"])
    with pytest.raises(LibError, match="not on the grid's curve"):
        FirmBook(usd, credit=lines["credit"])
    with pytest.raises(LibError, match="one row per column"):
        monte_carlo_revalue_firm_var_es(firm, chain["factor"][:55], FC.CHAIN_S, host=True)
    with pytest.raises(LibError, match="one row per column"):
        monte_carlo_revalue_firm_var_es(firm, FC.factor(32), FC.CHAIN_S, host=True)
    with pytest.raises(LibError):
        monte_carlo_revalue_firm_var_es(firm, chain["factor"], 0, host=True)
    with pytest.raises(LibError, match="shape"):
        revalue_shocks_firm(firm, chain["x"][:, :55], host=True)
    with pytest.raises(LibError, match="do not fit max_bytes"):
        monte_carlo_revalue_firm_var_es(firm, chain["factor"], FC.CHAIN_S, host=True, max_bytes=8 * 5 * (FC.CHAIN_S + 1))
    x = chain["x"][:4].copy()
    x[1, 36] = -(1.0 + firm.line("inflation").b0[0]) * 1e4 - 1.0           # the first breakeven to just below -100 %
    with pytest.raises(LibError, match=r"1 scenario\(s\) .* breakeven rate at or below -100 % .* first at index 1"):
        revalue_shocks_firm(firm, x, host=True)
    x[3, 33], x[0, 0] = np.nan, np.inf                                      # a spread shock and a quote that are not finite
    with pytest.raises(LibError, match=r"3 scenario\(s\) .* first at index 0"):
        revalue_shocks_firm(firm, x, host=True, max_bytes=8 * 5 * 5 + 2 * firm_scenario_bytes(firm))
    with pytest.raises(LibError, match=r"scenario\(s\) give a discount factor .* first at index \d+"):
        monte_carlo_revalue_firm_var_es(firm, chain["factor"] * 1e4, FC.CHAIN_S, seed=FC.SEED, host=True)
