"""reference deadtrees/data/deadtreedata.py -> deadtrees_amd.data.deadtreedata"""
from deadtrees_amd.data.deadtreedata import DeadtreeDatasetConfig, DeadtreesDataModule, train_transform, val_transform  # noqa: F401
from deadtrees_amd.data.shards import split_shards  # noqa: F401
