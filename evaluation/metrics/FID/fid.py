"""Drop-in for the reference's `evaluation/metrics/FID/fid.py` import path."""
from freefine_amd.metrics import calculate_fid, get_inception_activations, parse_data  # noqa: F401
