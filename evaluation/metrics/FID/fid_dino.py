"""Drop-in for the reference's `evaluation/metrics/FID/fid_dino.py` import path."""
from freefine_amd.metrics import calculate_fid_dino, parse_data  # noqa: F401
