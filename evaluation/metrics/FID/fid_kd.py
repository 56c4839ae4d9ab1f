"""Drop-in for the reference's `evaluation/metrics/FID/fid_kd.py` import path."""
from freefine_amd.metrics import calculate_fid_kd, parse_data  # noqa: F401
