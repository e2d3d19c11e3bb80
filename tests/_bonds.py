"""Bond books shared by the bond tests (inputs only; no expected values)."""
from adrates_amd.trades.market_data import random_bond_book as random_book  # noqa: F401


def scalar_measures(bond, curve, settle, clean_price=None, z=None):
    """The scalar host methods, in the order BondBook.measures evaluates them."""
    if z is None:
        z = bond.z_spread(settle, curve, clean_price)
    clean = bond.clean_price(settle, curve, z, settle)
    return {"z": z, "dirty": bond.dirty_price(settle, curve, z, settle), "clean": clean,
            "ytm": bond.yield_to_maturity(settle, clean), "duration": bond.duration(settle, curve, "macaulay", z),
            "convexity": bond.convexity(settle, curve, z), "dv01": bond.dv01(settle, curve, z)}
