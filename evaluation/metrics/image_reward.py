"""Drop-in for the reference's `evaluation/metrics/image_reward.py` import path."""
from freefine_amd.metrics import calculate_irs  # noqa: F401
