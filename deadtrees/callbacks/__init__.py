"""reference deadtrees/callbacks -> deadtrees_amd.callbacks"""
