"""Drop-in for the reference's `evaluation/metrics/MD/mean_distance.py` import path."""
from freefine_amd.metrics import calculate_md, mean_distance, transform_coordinates  # noqa: F401
