"""Price indices (cavour/market/indices/)."""
from .inflation_index import InflationIndex  # noqa: F401
