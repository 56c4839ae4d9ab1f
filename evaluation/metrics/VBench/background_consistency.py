"""Drop-in for the reference's `evaluation/metrics/VBench/background_consistency.py` import path."""
from freefine_amd.metrics import calculate_bgc, consistency_pairs as parse_data  # noqa: F401
