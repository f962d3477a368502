"""Volume pre/post-processing of the reference's ``datasets`` package that runs on the device (datasets/common.py)."""
