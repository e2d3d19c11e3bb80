"""Delta-gamma P&L from ladders on the CPU: the host twin adr_ladder_pnl_host against exact rational arithmetic, its exact
cases, bit contract and refusals, and `delta_gamma_sub_books` against full revaluation on the host twins (no GPU)."""
import numpy as np
import pytest

from adrates_amd import _native
from adrates_amd.market.position.engine import Engine
from adrates_amd.market.position.ladder_pnl import delta_gamma_sub_books, ladder_pnl, ladder_rows, shock_matrix_bp
from adrates_amd.market.position.scenarios import revalue_on_curves_sub_books
from adrates_amd.utils.error import LibError

from . import _ladder_pnl_cases as C

ALL = (True, True, True)


def host(ladders, shocks, want=ALL):
    return _native.ladder_pnl_host(ladders, shocks, want)


@pytest.mark.parametrize("P,S,B", C.EXACT_TABLES)
def test_host_twin_against_exact_arithmetic(P, S, B):
    """|got - exact| <= (P^2 + P + 8) 2^-53 gross, for pnl and for each part on its own gross.  Observed worst share of
    the bound: 0.23 at P = 1, 5.2e-3 at P = 32, 9.5e-5 at P = 256."""
    ladders, shocks = C.table(P, S, B)
    got = host(ladders, shocks)
    worst = C.worst_error(P, S, B, got)
    print(f"host twin, P = {P}, S = {S}, B = {B}: worst error {worst:.2e} of the bound")
    assert worst <= 1.0
    assert C.same_bits(got["pnl"], got["delta_pnl"] + got["gamma_pnl"])
    # through the Python layer: the same bits, and the PV slot does not matter
    delta, gamma = C.split(ladders, P)
    assert C.same_bits(ladder_pnl(delta, gamma, shocks, host=True), got["pnl"])
    if P <= 64:
        assert C.same_bits(ladder_pnl(delta, None, shocks, host=True), got["delta_pnl"])
        assert np.allclose(got["pnl"], delta @ shocks.T + 0.5 * np.einsum("sp,bpq,sq->bs", shocks, gamma, shocks), rtol=1e-9)


def test_exact_cases():
    P, S, B = 33, 65, 9
    ladders, shocks = C.table(P, S, B, seed=1)
    ladders[:, 0] = np.nan                                  # the PV slot is not read
    base = host(ladders, shocks)
    assert all(np.all(np.isfinite(base[k])) for k in C.PARTS)
    zero_row = ladders.copy()
    zero_row[4, 1:] = 0.0
    got = host(zero_row, shocks)
    for k in C.PARTS:
        assert np.all(got[k][4] == 0.0) and C.same_bits(np.delete(got[k], 4, 0), np.delete(base[k], 4, 0)), k
    zero_shock = shocks.copy()
    zero_shock[63] = 0.0
    got = host(ladders, zero_shock)
    for k in C.PARTS:
        assert np.all(got[k][:, 63] == 0.0) and C.same_bits(np.delete(got[k], 63, 1), np.delete(base[k], 63, 1)), k
    for slot in (1 + 5, 1 + P + 7 * P + 2):                 # a NaN in the desk's delta, then in its gamma
        bad = ladders.copy()
        bad[2, slot] = np.nan
        got = host(bad, shocks)
        assert np.all(np.isnan(got["pnl"][2]))
        for k in C.PARTS:
            assert C.same_bits(np.delete(got[k], 2, 0), np.delete(base[k], 2, 0)), (slot, k)
    # a gamma that is not symmetric is used as given: its transpose gives the same quadratic form only up to rounding,
    # and one entry alone moves the P&L by 1/2 gamma_pq x_p x_q
    one = np.zeros((1, 1 + P + P * P))
    one[0, 1 + P + 3 * P + 5] = 2.0
    assert np.array_equal(host(one, shocks)["pnl"][0], shocks[:, 3] * shocks[:, 5])


@pytest.mark.parametrize("P", C.PILLARS)
def test_host_bit_contract(P):
    """pnl[b][s] depends on ladder row b and shock row s alone: desks and scenarios alone, in every count of the
    geometry, permuted, and twice."""
    B, S = (73, 129) if P < 256 else (9, 5)
    ladders, shocks = C.table(P, S, B, seed=2)
    got = host(ladders, shocks)
    assert all(C.same_bits(got[k], v) for k, v in host(ladders, shocks).items()), "two runs"
    for b in {0, 7, 8, B - 1}:
        alone = host(ladders[b:b + 1], shocks)
        assert all(C.same_bits(alone[k][0], got[k][b]) for k in C.PARTS), f"desk {b} alone"
    for s in {0, 3, S - 1}:
        alone = host(ladders, shocks[s:s + 1])
        assert all(C.same_bits(alone[k][:, 0], got[k][:, s]) for k in C.PARTS), f"scenario {s} alone"
    for nb in C.DESKS:
        for ns in C.SCENARIOS:
            if nb <= B and ns <= S and P <= 33:
                part = host(ladders[B - nb:], shocks[S - ns:], (True, False, False))["pnl"]
                assert C.same_bits(part, got["pnl"][B - nb:, S - ns:]), (nb, ns)
    rng = np.random.default_rng(5)
    pb, ps = rng.permutation(B), rng.permutation(S)
    moved = host(ladders[pb], shocks[ps])
    assert all(C.same_bits(moved[k], got[k][pb][:, ps]) for k in C.PARTS), "rows permuted"
    only = host(ladders, shocks, (False, False, True))
    assert list(only) == ["gamma_pnl"] and C.same_bits(only["gamma_pnl"], got["gamma_pnl"])


def test_host_refusals():
    lib = _native.load()
    ok_l, ok_x = C.table(3, 2, 2)
    status = lambda *a, **k: pytest.raises(LibError, *a, **k)
    with status() as e:
        host(np.zeros((2, 1)), np.zeros((2, 0)))            # P = 0
    assert e.value.status == -1
    with status() as e:
        host(np.zeros((1, 1 + 257 + 257 * 257)), np.zeros((1, 257)))
    assert e.value.status == -2 and "257" in str(e.value)
    with status() as e:
        host(ok_l, np.zeros((0, 3)))                        # S = 0
    assert e.value.status == -1
    with status() as e:
        host(ok_l, ok_x, (False, False, False))
    assert e.value.status == -1 and "no output" in str(e.value)
    out = np.empty((2, 2))
    p = _native._ptr
    assert lib.adr_ladder_pnl_host(2, 3, None, 2, p(ok_x), p(out), None, None) == -1
    assert lib.adr_ladder_pnl_host(2, 3, p(ok_l), 2, None, p(out), None, None) == -1
    assert lib.adr_ladder_pnl_host(-1, 3, p(ok_l), 2, p(ok_x), p(out), None, None) == -1
    out[:] = -7.25
    assert lib.adr_ladder_pnl_host(0, 3, None, 2, p(ok_x), p(out), None, None) == 0 and np.all(out == -7.25)      # B = 0
    assert host(np.zeros((0, 13)), ok_x)["pnl"].shape == (0, 2)
    assert lib.adr_ladder_pnl_host(2, 256, None, 2, None, None, None, None) == -1
    # the Python layer's own shape checks
    for args in ((np.zeros((2, 3)), np.zeros((2, 3, 2)), ok_x), (np.zeros((2, 3)), None, np.zeros((2, 4))), (np.zeros(3), None, ok_x)):
        with pytest.raises(LibError):
            ladder_pnl(*args, host=True)
    assert ladder_rows(np.ones((2, 3))).shape == (2, 13)


def test_shock_matrix():
    tenors = ["1Y", "2Y", "5Y"]
    got = shock_matrix_bp(tenors, [0.04, {"2Y": -0.1}, {"7Y": 1.0}, 0.0], 100.0)
    assert np.array_equal(got, [[4.0, 4.0, 4.0], [0.0, -10.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    assert shock_matrix_bp(tenors, [], 1.0).shape == (0, 3)


@pytest.fixture(scope="module")
def mixed():
    return C.L.mixed_book()


@pytest.mark.parametrize("interp", C.SCHEMES)
def test_delta_gamma_against_full_revaluation(interp, mixed):
    """The residual of the delta-gamma P&L against full revaluation is third order in the shock, that of delta alone
    second order, per desk and direction: the gamma ladders and the scenario code agree with each other.  Observed on the
    host twins - delta-gamma ratio, delta-only ratio: LINEAR_ZERO_RATES 7.752 - 8.010, 3.669 - 4.033; FLAT_FWD_RATES
    7.751 - 8.009, 3.512 - 4.035; LINEAR_FWD_RATES 7.953 - 8.023, 3.971 - 4.016."""
    model, ir = C.gbp(interp)
    n = mixed.n_trades
    keys = C.desk_keys(n)
    x = C.shock_rows(len(ir.swap_rates))
    times, dfs = C.shocked_dfs(ir, x)
    sub = revalue_on_curves_sub_books(interp, times, dfs, mixed, keys, C.VD, host=True)
    full = sub["sub_pv"][:, :-1] - sub["sub_pv"][:, -1:]
    dg = delta_gamma_sub_books(Engine(model), ir, mixed, keys, x, parts=True, host=True)
    assert dg["labels"] == sub["labels"] == [0, 1, 3, 4, 5] and dg["pnl"].shape == full.shape == (5, 10)
    assert C.same_bits(dg["pnl"], dg["delta_pnl"] + dg["gamma_pnl"])
    C.check_orders(full, dg["delta_pnl"], dg["gamma_pnl"], f"host, {interp.name}")
    # the ladders the P&L came from are price_sub_books', and without the parts the dict holds the P&L alone
    plain = delta_gamma_sub_books(Engine(model), ir, mixed, keys, x, host=True)
    assert "delta_pnl" not in plain and C.same_bits(plain["pnl"], dg["pnl"]) and plain["delta"].shape == (5, x.shape[1])
    assert C.same_bits(ladder_pnl(dg["delta"], dg["gamma"], x, host=True), dg["pnl"])
