"""Drop-in for the reference's `evaluation/metrics/VBench/subject_consistency.py` import path."""
from freefine_amd.metrics import calculate_subc, consistency_pairs as parse_data  # noqa: F401
