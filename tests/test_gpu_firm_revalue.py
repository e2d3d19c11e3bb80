"""Full revaluation of a firm on the GPU (market/position/monte_carlo_firm.py; adr_shock_columns_dev and
adr_scenario_rows_merge_dev between the bootstrap, the three sub-book launches and the tail entries), on the firm of
tests/_firm_revalue_cases.py: the chain against `combine_sub_book_rows` of the three device ``*_on_curves_sub_books`` calls on
the twin's rows, whatever the tiling, its tail figures against the tail entries, the device against the host chain, bad
scenarios, the explain dict and the third-order gap to delta-gamma."""
import numpy as np
import pytest

from adrates_amd.market.position.engine import Engine
from adrates_amd.market.position.ladder_pnl import augmented_ladder_pnl
from adrates_amd.market.position.monte_carlo import allocate_tail_select, monte_carlo_shocks, monte_carlo_var_es, tail_measures_select
from adrates_amd.market.position.monte_carlo_firm import (firm_ladders, firm_scenario_bytes, monte_carlo_explain_firm_var_es,
                                                          monte_carlo_revalue_firm_var_es, revalue_shocks_firm)
from adrates_amd.market.position.scenarios import combine_sub_book_rows, tail_count
from adrates_amd.utils.error import LibError

from . import _firm_revalue_cases as FC
from . import _tail_alloc_cases as TA
from ._parity import REL_TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def chain(gpu_ctx):
    """The recipe, the three-line firm, its factor, the DEVICE's joint shock rows and the device chain's P&L, made once."""
    curves = FC.curves(gpu_ctx)
    firm = FC.firm(curves)
    factor = FC.factor(firm.n_columns)
    x = monte_carlo_shocks(factor, FC.CHAIN_S, FC.SEED, ctx=gpu_ctx)
    yield dict(curves=curves, firm=firm, factor=factor, x=x, pnl=revalue_shocks_firm(firm, x), engine=Engine(FC.model()[0]))
    curves.close()


def test_chain_has_the_bits_of_the_three_lines_combined(gpu_ctx, chain):
    assert chain["pnl"]["labels"] == FC.LABELS and chain["pnl"]["pnl"].shape == (5, FC.CHAIN_S)
    want = combine_sub_book_rows(FC.line_rows(chain["curves"], chain["firm"], chain["x"], host=False, ctx=gpu_ctx))
    assert want["labels"] == FC.LABELS
    assert np.array_equal(FC.bits(chain["pnl"]["pnl"]), FC.bits(want["rows"][:, :-1] - want["rows"][:, -1:]))


def test_chain_does_not_depend_on_the_tiling(chain):
    firm = chain["firm"]
    per, rows = firm_scenario_bytes(firm), 8 * 5 * (FC.CHAIN_S + 1)
    for tile in FC.TILES:
        got = revalue_shocks_firm(firm, chain["x"], max_bytes=rows + tile * per)
        assert np.array_equal(FC.bits(got["pnl"]), FC.bits(chain["pnl"]["pnl"])), tile
    x = chain["x"][:5].copy()
    x[2] = 0.0
    pnl = revalue_shocks_firm(firm, x)["pnl"]
    assert np.array_equal(FC.bits(pnl[:, 2]), FC.bits(np.zeros(5))) and np.all(pnl[:, [0, 1, 3, 4]] != 0.0), "a zero shock row"


@pytest.mark.parametrize("kind", ["rates", "credit", "inflation"])
def test_one_line_is_that_lines_own_call(gpu_ctx, chain, kind):
    curves = chain["curves"]
    firm = FC.firm(curves, kind)
    cols = chain["firm"].columns
    keep = list(cols["curve"]) + {"rates": [], "credit": list(cols["spread"]), "inflation": list(cols["breakeven"])}[kind]
    x = np.ascontiguousarray(chain["x"][:, keep])
    got = revalue_shocks_firm(firm, x)
    (labels, rows), = FC.line_rows(curves, firm, x, host=False, ctx=gpu_ctx, kinds=(kind,))
    assert got["labels"] == labels and np.array_equal(FC.bits(got["pnl"]), FC.bits(rows[:, :-1] - rows[:, -1:]))


def test_var_es_and_allocation_are_the_tail_entries_of_the_rows(chain):
    firm, pnl = chain["firm"], chain["pnl"]["pnl"]
    per = firm_scenario_bytes(firm)
    for level in (0.99, 0.9):
        var, es = tail_measures_select(pnl, level, host=True)
        whole = allocate_tail_select(pnl, level, host=True)
        for max_bytes in (2 ** 31, 8 * 5 * (FC.CHAIN_S + 1) + 64 * per):
            got = monte_carlo_revalue_firm_var_es(firm, chain["factor"], FC.CHAIN_S, level=level, seed=FC.SEED, max_bytes=max_bytes)
            assert sorted(got) == ["es", "labels", "var"] and got["labels"] == FC.LABELS
            assert np.array_equal(FC.bits(got["var"]), FC.bits(var)) and np.array_equal(FC.bits(got["es"]), FC.bits(es)), level
        got = monte_carlo_revalue_firm_var_es(firm, chain["factor"], FC.CHAIN_S, level=level, seed=FC.SEED, allocate=True)
        assert np.array_equal(FC.bits(got["var"]), FC.bits(var)) and np.array_equal(FC.bits(got["es"]), FC.bits(es))
        assert got["firm_var"] == whole["var"] and got["firm_es"] == whole["es"]
        assert np.array_equal(FC.bits(got["comp_var"]), FC.bits(whole["comp_var"]))
        assert np.array_equal(FC.bits(got["comp_es"]), FC.bits(whole["comp_es"]))
        TA.check(dict(var=got["firm_var"], es=got["firm_es"], comp_var=got["comp_var"], comp_es=got["comp_es"]), pnl, -1,
                 tail_count(level, FC.CHAIN_S))


def test_device_chain_against_the_host_chain(chain):
    """`test_gpu_monte_carlo_revalue.test_device_chain_against_the_host_chain`'s bound on the firm's desks: on the same
    joint rows the two chains differ by the pricing kernels' exp, log and pow alone; each desk PV is held to REL_TOL max(N,
    |PV|), N the desk's summed notionals over its lines and PV the desk's own (the lines' sum), and a P&L, the difference of
    the scenario's PV and the base's, to the sum of their two bounds."""
    curves, firm = chain["curves"], chain["firm"]
    host = revalue_shocks_firm(firm, chain["x"], host=True)
    pv = np.abs(combine_sub_book_rows(FC.line_rows(curves, firm, chain["x"]))["rows"])
    N = FC.desk_notionals(firm)[:, None]
    bound = REL_TOL * (np.maximum(N, pv[:, :-1]) + np.maximum(N, pv[:, -1:]))
    err = np.abs(chain["pnl"]["pnl"] - host["pnl"])
    print("device against host chain, worst share of the bound per desk:", np.max(err / bound, axis=1))
    assert host["labels"] == chain["pnl"]["labels"] and np.all(N > 0.0) and np.all(err <= bound)


def test_bad_scenarios_raise(chain):
    firm = chain["firm"]
    with pytest.raises(LibError, match=r"scenario\(s\) give a discount factor .* first at index \d+"):
        monte_carlo_revalue_firm_var_es(firm, chain["factor"] * 1e4, FC.CHAIN_S, seed=FC.SEED)
    x = chain["x"][:4].copy()
    x[1, 36] = -(1.0 + firm.line("inflation").b0[0]) * 1e4 - 1.0           # the first breakeven to just below -100 %
    with pytest.raises(LibError, match=r"1 scenario\(s\) .* breakeven rate at or below -100 % .* first at index 1"):
        revalue_shocks_firm(firm, x)
    x[3, 33], x[0, 0] = np.nan, np.inf                                      # a spread shock and a quote that are not finite
    with pytest.raises(LibError, match=r"3 scenario\(s\) .* first at index 0"):
        revalue_shocks_firm(firm, x, max_bytes=8 * 5 * 5 + 2 * firm_scenario_bytes(firm))
    with pytest.raises(LibError, match="do not fit max_bytes"):
        monte_carlo_revalue_firm_var_es(firm, chain["factor"], FC.CHAIN_S, max_bytes=8 * 5 * (FC.CHAIN_S + 1))
    with pytest.raises(LibError, match="one row per column"):
        monte_carlo_revalue_firm_var_es(firm, chain["factor"][:55], FC.CHAIN_S)


def test_explain_sets_the_two_routes_side_by_side(gpu_ctx, chain):
    firm, L, engine = chain["firm"], chain["factor"], chain["engine"]
    got = monte_carlo_explain_firm_var_es(engine, firm, L, FC.CHAIN_S, level=0.9, seed=FC.SEED)
    full = monte_carlo_revalue_firm_var_es(firm, L, FC.CHAIN_S, level=0.9, seed=FC.SEED)
    dg = monte_carlo_var_es(None, None, L, FC.CHAIN_S, level=0.9, seed=FC.SEED, ctx=gpu_ctx, ladders=firm_ladders(engine, firm))
    assert got["labels"] == full["labels"] == FC.LABELS
    for key, ref in (("full_var", full["var"]), ("full_es", full["es"]), ("dg_var", dg["var"]), ("dg_es", dg["es"]),
                     ("gap_var", full["var"] - dg["var"]), ("gap_es", full["es"] - dg["es"])):
        assert np.array_equal(FC.bits(got[key]), FC.bits(ref)), key
    assert np.all(np.abs(got["gap_var"]) < 0.05 * np.abs(got["full_var"]))


# ------------------------------------------------------------------------------------------ the reason for the feature
@pytest.mark.parametrize("kinds", [("credit",), ("inflation",), ()], ids=["credit", "inflation", "three_lines"])
def test_gap_to_delta_gamma_is_third_order(gpu_ctx, chain, kinds):
    """The same seed with the factor L and with L / 2: the rows are exact halves, and the worst |full - delta-gamma| over
    the scenarios, per desk, falls by about 8 - inside GAP_BAND for every desk, none dropped (the host twins: 7.9 to 8.1,
    tests/test_firm_revalue_host.py)."""
    firm = chain["firm"] if not kinds else FC.firm(chain["curves"], *kinds)
    L = FC.factor(firm.n_columns)
    x, half = (monte_carlo_shocks(s * L, FC.CHAIN_S, FC.SEED, ctx=gpu_ctx) for s in (1.0, 0.5))
    assert np.array_equal(FC.bits(half), FC.bits(0.5 * x))
    rows = firm_ladders(chain["engine"], firm)
    gap = [(revalue_shocks_firm(firm, s)["pnl"], augmented_ladder_pnl(rows, s, ctx=gpu_ctx)) for s in (x, half)]
    ratios = FC.gap_ratios(*gap[0], *gap[1])
    print("device: gap ratios per desk", firm.labels, np.round(ratios, 3))
    assert ratios.shape == (firm.n_desks,) and np.all((FC.GAP_BAND[0] < ratios) & (ratios < FC.GAP_BAND[1])), ratios
