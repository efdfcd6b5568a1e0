"""reference deadtrees/callbacks/multistage.py -> deadtrees_amd.callbacks.multistage"""
from deadtrees_amd.callbacks.multistage import MultiStage  # noqa: F401
