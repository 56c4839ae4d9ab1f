"""Drop-in for the reference's `evaluation/metrics/human_preference_score.py` import path."""
from freefine_amd.metrics import calculate_hps  # noqa: F401
